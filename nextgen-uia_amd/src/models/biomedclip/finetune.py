"""BiomedCLIP contrastive fine-tuning on the MI355X HIP path — drop-in for /root/reference/src/models/biomedclip/finetune.py.

Same command line (every flag and default of reference :32-111), same loop semantics (:211-361): micro-batch InfoNCE,
(loss / accumulation_steps).backward(), non-finite batches skipped, clip_grad_norm_ → AdamW → cosine LR once per cycle,
validation each epoch, best-val checkpoint of the adapter parameters only (names containing "mona"/"lora", :200-208),
early stopping, runs/<exp>/{log.log,best_model.pth}.  Added, non-breaking: --dtype {bf16,fp32}, --synthetic / --data_pt / --finetune_root (the reference's caption folders as released), --tokenizer_json (real token ids),
--ckpt_path (an open_clip BiomedCLIP state dict; without it the towers are randomly initialised because the build image
has no network), and data parallelism when launched under torch.distributed.run (one process per GPU, one RCCL
all-reduce of the flat adapter-gradient buffer per optimiser update ≡ the reference's accumulation).

What differs underneath: encode_image / encode_text / loss / backward / optimiser run in libuia_hip.so (uia_hip.*); the loop is
src/models/contrastive.py with its BIOMEDCLIP recipe, this module keeps the flags and the model.
`--method full` (the reference's default): the image tower trains through op-level functions with `uia_wgrad` weight gradients
(all blocks or --tune_layers last3/6/9, lr forced to 1e-6 as in reference :153-155, whole state dict checkpointed); with
--tune_text_encoder the BERT weights, LayerNorms and embedding tables train as well (`uia_embed_bwd`).
"""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_lora_to_biomedclip, inject_mona_variant_to_open_clip
from src.models import contrastive
from src.third_party.biomedclip.model import SyntheticTokenizer, create_biomedclip
from src.utils import tokenizer_file
from src.utils.tools import default_device, parse_config


def get_args(argv=None):
    p = argparse.ArgumentParser("BiomedCLIP Fine-tuning")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--exp", type=str, default="biomedclip_finetune")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--ckpt", type=str, default=None, help="Path to finetuned model checkpoint")
    p.add_argument("--method", type=str, default="full", choices=["full", "mona", "lora"])
    p.add_argument("--tune_text_encoder", default=False, action="store_true")
    p.add_argument("--tune_layers", type=str, default="all", choices=["last3", "last6", "last9", "all"])
    p.add_argument("--mona_variant", type=str, default="freq_enhanced", choices=["baseline", "fractional", "noise_aware", "freq_enhanced", "hybrid"])
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--lora_r", type=int, default=16)
    p.add_argument("--lora_alpha", type=int, default=32)
    p.add_argument("--lora_dropout", type=float, default=0.1)
    p.add_argument("--lora_layers", type=int, default=None)
    p.add_argument("--temperature", type=float, default=0.07)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=32)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_min", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--beta1_adam", type=float, default=0.9)
    p.add_argument("--beta2_adam", type=float, default=0.95)
    p.add_argument("--device", type=str, default=default_device())       # decided without a HIP call: the loader workers fork first
    p.add_argument("--patience", type=int, default=10)
    p.add_argument("--accumulation_steps", type=int, default=4)
    p.add_argument("--grad_clip", type=float, default=1.0)
    # additions of this build
    contrastive.add_build_args(p)
    p.add_argument("--ckpt_path", type=str, default=None, help="open_clip BiomedCLIP state dict (.pt); random init if absent")
    p.add_argument("--stats_json", type=str, default=None, help="write train()'s return value (per-epoch wall time and update counts included) to this file")
    return p.parse_args(argv)


def make_tokenizer(args):
    tc = {} if not args.model_config else parse_config(args.model_config)["text_cfg"]
    context = tc.get("max_position_embeddings", 256)
    return tokenizer_file.from_args(args, context, tc.get("vocab_size", 30522), pools_at_argmax=False) or SyntheticTokenizer(context)


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    model = create_biomedclip(state_dict=state, config=cfg, seed=args.seed)
    tokenizer = make_tokenizer(args)
    model.float()
    if args.method == "full":                                    # reference :134-157
        if not args.tune_text_encoder:
            for p in model.text.parameters():
                p.requires_grad = False
            logging.info("Text encoder frozen")
        if args.tune_layers != "all":
            blocks = model.visual.trunk.blocks
            for p in model.visual.parameters():
                p.requires_grad = False
            layers = {"last3": 3, "last6": 6, "last9": 9}.get(args.tune_layers, 0)
            for i in range(len(blocks) - layers, len(blocks)):
                for p in blocks[i].parameters():
                    p.requires_grad = True
            logging.info(f"Tuning ViT layers {len(blocks) - layers}-{len(blocks) - 1} ({layers}/{len(blocks)} layers)")
        if args.lr > 1e-5:
            args.lr = 1e-6
            logging.info(f"Adjusted learning rate to {args.lr} for full fine-tuning")
        if hasattr(model, "logit_scale"):
            model.logit_scale.requires_grad = False              # not used by the InfoNCE loss (fixed temperature): no gradient ever reaches it
        model.to(args.device)
        tr = sum(p.numel() for p in model.parameters() if p.requires_grad)
        tot = sum(p.numel() for p in model.parameters())
        logging.info(f"Trainable parameters: {tr:,} / {tot:,} ({100 * tr / tot:.2f}%)")
        return model, tokenizer
    for p in model.parameters():
        p.requires_grad = False
    if args.method == "mona":
        inject_mona_variant_to_open_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        key = "mona"
        logging.info(f"MONA variant: {args.mona_variant}, bottleneck: {args.mona_bottleneck}")
    else:
        inject_lora_to_biomedclip(model, lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=args.lora_dropout,
                                  num_layers=args.lora_layers, tune_text_encoder=args.tune_text_encoder)
        key = "lora"
        logging.info(f"LoRA rank: {args.lora_r}, alpha: {args.lora_alpha}, dropout: {args.lora_dropout}")
    for name, p in model.named_parameters():
        if key in name.lower():
            p.requires_grad = True
    model.to(args.device)
    tr = sum(p.numel() for p in model.parameters() if p.requires_grad)
    tot = sum(p.numel() for p in model.parameters())
    logging.info(f"Trainable parameters: {tr:,} / {tot:,} ({100 * tr / tot:.2f}%)")
    return model, tokenizer


RECIPE = contrastive.BIOMEDCLIP


def train(args):
    return contrastive.train(args, RECIPE, prepare_model, make_tokenizer)


def main(argv=None):
    return contrastive.run(get_args(argv), RECIPE, prepare_model, make_tokenizer)


if __name__ == "__main__":
    main()
