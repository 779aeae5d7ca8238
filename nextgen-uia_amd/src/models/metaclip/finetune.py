"""MetaCLIP contrastive fine-tuning with Mona adapters on the MI355X HIP path — drop-in for
/root/reference/src/models/metaclip/finetune.py (the clip/ and unimedclip/ entry points of the reference repeat its loop).

Same command line (every flag and default of reference :26-64; default --mona_variant noise_aware, batch 64, no gradient
accumulation) and loop semantics (:92-218): per batch InfoNCE on L2-normalised features, non-finite batches skipped,
clip_grad_norm_(1.0) → AdamW → cosine LR every iteration, a validation pass per epoch in eval mode, best-val checkpoint of
the parameters whose name contains "mona", early stopping by --patience, runs/<exp>/{log.log,best_model.pth}.
Added, non-breaking: --dtype, --synthetic / --data_pt / --finetune_root (the reference's caption folders as released), --tokenizer_json (real token ids), --ckpt_path, --model_config, data parallelism under
torch.distributed.run, and --zero_shot_eval: the reference's post-training zero-shot evaluation (run_zero_shot_evaluation, :240-296), which the
reference always runs, is opt-in here — rank 0 starts src/models/metaclip/zero_shot.py once per dataset, each a fresh child process.
The loop is src/models/contrastive.py with its CLIP_FAMILY recipe; this module keeps the flags and the model.
"""
import argparse
import dataclasses
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_open_clip
from src.models import contrastive
from src.third_party.open_clip.model import SyntheticClipTokenizer, create_metaclip
from src.utils import tokenizer_file
from src.utils.tools import default_device, parse_config


def get_args(argv=None):
    p = argparse.ArgumentParser("MetaCLIP Fine-tuning with Frequency-Enhanced MONA")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("--exp", type=str, default="metaclip_finetune")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--mona_variant", type=str, default="noise_aware")
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--temperature", type=float, default=0.07)
    p.add_argument("--uniformity_weight", type=float, default=0)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_min", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--beta1_adam", type=float, default=0.9)
    p.add_argument("--beta2_adam", type=float, default=0.95)
    p.add_argument("--device", type=str, default=default_device())       # decided without a HIP call: the loader workers fork first
    p.add_argument("--patience", type=int, default=10)
    # additions of this build
    contrastive.add_build_args(p)
    p.add_argument("--ckpt_path", type=str, default=None, help="open_clip state dict (.pt); random init if absent")
    contrastive.add_zero_shot_flags(p)
    return p.parse_args(argv)


def make_tokenizer(args):
    tc = ((parse_config(args.model_config) if args.model_config else None) or {}).get("text_cfg", {})
    context, vocab = tc.get("context_length", 77), tc.get("vocab_size", 49408)
    return tokenizer_file.from_args(args, context, vocab, pools_at_argmax=True) or SyntheticClipTokenizer(context, vocab)


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    model = create_metaclip(state_dict=state, config=cfg, seed=args.seed)
    tokenizer = make_tokenizer(args)
    for p in model.parameters():
        p.requires_grad = False
    model, mona_count = inject_mona_variant_to_open_clip(model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck,
                                                         num_layers=args.mona_layers)
    for name, p in model.named_parameters():
        if "mona" in name.lower():
            p.requires_grad = True
    model.float()
    model.to(args.device)
    return model, tokenizer


RECIPE = dataclasses.replace(contrastive.CLIP_FAMILY, zero_shot_script=Path(__file__).parent / "zero_shot.py",
                             zero_shot_flags=lambda args: ["--ckpt_path", args.ckpt_path] if args.ckpt_path else [])


def train(args):
    return contrastive.train(args, RECIPE, prepare_model, make_tokenizer)


def main(argv=None):
    return contrastive.run(get_args(argv), RECIPE, prepare_model, make_tokenizer)


if __name__ == "__main__":
    main()
