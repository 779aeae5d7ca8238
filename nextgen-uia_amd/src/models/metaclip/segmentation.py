"""MetaCLIP segmentation with the feature-pyramid adapter on the HIP path — counterpart of the reference's src/models/metaclip/segmentation.py.

Its command line (:28-67: default --mona_variant noise_aware, 1000 epochs, no LoRA flags) and model preparation (:74-121: the timm-trunk MetaCLIP, optional
Mona adapters loaded by name, TimmCLIPAdapter(task="seg") on layers 3/6/9, freeze_clip_backbone()); the loop is src/models/supervised.py with its SEGMENTATION
task and the reference's second early-stopping line (:222-223), the checkpoint {"reduces", "blocks", "seg_head", "mona"}, and test() writes the
visualize_seg pictures of the test split (--no-viz: none).  Data: `--synthetic` or `--data_pt` (src/datasets/segmentation.py)."""
import argparse
import dataclasses
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_mona_variant_to_open_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.models import supervised
from src.third_party.open_clip.model import create_metaclip
from src.third_party.timm.clip_adapter import TimmCLIPAdapter
from src.utils.tools import default_device, parse_config

TASK = dataclasses.replace(supervised.SEGMENTATION, stop_twice=True)


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="metaclip_seg")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--mona_variant", type=str, default="noise_aware")
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


criterion = TASK.criterion                                       # reference :71: DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)


def prepare_model(args):
    """reference :74-121."""
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    clip_model = create_metaclip(state_dict=state, config=cfg, seed=args.seed)
    clip_model.float()
    if args.mona_weights:
        inject_mona_variant_to_open_clip(clip_model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(clip_model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} pretrained MONA parameters from {args.mona_weights}")
    adapter = TimmCLIPAdapter(clip_model=clip_model, extract_layers=supervised.extract_layers(args), reduce_dim=args.reduce_dim, num_classes=args.num_classes,
                              img_size=args.img_size, patch_size=args.patch_size, task="seg")
    adapter.to(args.device)
    adapter.freeze_clip_backbone()
    return adapter


def train(args, prepare=None):
    """prepare: args -> model (default: this entry point's prepare_model)."""
    return supervised.train(args, TASK, prepare or prepare_model)


def test(args, prepare=None):
    return supervised.test(args, TASK, prepare or prepare_model)


def main(argv=None):
    return supervised.run(get_args(argv), TASK, prepare_model)


if __name__ == "__main__":
    main()
