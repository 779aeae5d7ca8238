"""UniMed-CLIP supervised classification on the HIP path — counterpart of the reference's src/models/unimedclip/classification.py.

Its command line (:29-70: --version ViT-B-16-quickgelu, --ckpt ckpt/unimed_clip_vit_b16.pt, default --mona_variant noise_aware, 1000 epochs, no LoRA flags)
and model preparation (:76-140: open_clip's NATIVE tower with QuickGELU forced, the checkpoint's `visual.*` keys and `logit_scale` loaded strict=False,
optional Mona adapters loaded by name, TimmCLIPAdapter(task="cls") on layers 3/6/9, freeze_clip_backbone()); the loop is that of
src/models/supervised.py.  The native tower has `visual.transformer` with batch-first blocks: the adapter feeds them the batch-first
tokens as they are (classification, note C-cls-1).  --ckpt_path, when given, takes the place of --ckpt."""
import argparse
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_open_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.models import supervised
from src.third_party.open_clip.model import create_native_clip
from src.third_party.timm.clip_adapter import TimmCLIPAdapter
from src.utils.tools import default_device, parse_config


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="unimedclip_cls")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--version", type=str, default="ViT-B-16-quickgelu")
    p.add_argument("--ckpt", type=str, default="ckpt/unimed_clip_vit_b16.pt")
    p.add_argument("--mona_variant", type=str, default="noise_aware")
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--reduce_dim", type=int, default=512)
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_min", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.95)
    p.add_argument("--device", type=str, default=default_device())
    p.add_argument("--patience", type=int, default=15)
    p.add_argument("--test", default=False, action="store_true")
    supervised.add_build_args(p)
    return p.parse_args(argv)


def prepare_model(args):
    """reference :76-140."""
    cfg = parse_config(args.model_config) if args.model_config else None
    clip_model = create_native_clip(args.version, config=cfg, seed=args.seed, force_quick_gelu=True)
    ckpt = args.ckpt_path or args.ckpt
    if ckpt and os.path.exists(ckpt):
        checkpoint = torch.load(ckpt, map_location="cpu", weights_only=False)
        state_dict = checkpoint["state_dict"] if "state_dict" in checkpoint else checkpoint
        state_dict = {k.replace("module.", ""): v for k, v in state_dict.items()}
        visual_state_dict = {k: v for k, v in state_dict.items() if k.startswith("visual.") or k == "logit_scale"}
        clip_model.load_state_dict(visual_state_dict, strict=False)
        logging.info(f"loaded {len(visual_state_dict)} visual tensors from {ckpt}")
    else:
        logging.info(f"checkpoint {ckpt} not found: randomly initialised {args.version}")
    clip_model.float()
    if args.mona_weights:
        inject_mona_variant_to_open_clip(clip_model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(clip_model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} pretrained MONA parameters from {args.mona_weights}")
    adapter = TimmCLIPAdapter(clip_model=clip_model, extract_layers=supervised.extract_layers(args), reduce_dim=args.reduce_dim, num_classes=args.num_classes,
                              img_size=args.img_size, patch_size=args.patch_size, task="cls")
    adapter.to(args.device)
    adapter.freeze_clip_backbone()
    return adapter


def main(argv=None):
    return supervised.run(get_args(argv), supervised.CLASSIFICATION, prepare_model)


if __name__ == "__main__":
    main()
