"""The from-scratch UNet segmentation baseline on the HIP path — counterpart of the reference's src/models/baselines/segmentation.py (step 2
of scripts/baselines.sh, the yardstick of the paper's Dice / HD95 tables).

Kept: the command line (exp unet_seg, img_size 224, batch 32, 200 epochs, patience 15, AdamW 1e-4 / betas 0.9, 0.95 / weight decay 0.01, cosine
per iteration to --lr_min, no clipping), prepare_model = UNet(args.in_channels, args.num_classes) with every parameter trainable, DiceCE per
iteration, validation every 10 epochs and at the last one with best-by-Dice, early stopping by --patience, a test pass after each validation,
the checkpoint `model.state_dict()` (BatchNorm buffers included) under runs/<exp>/<dataset>/train, and the Dice / IoU / HD95 / ASD table with
results.csv under runs/<exp>/<dataset>/test.
The loop is src/models/supervised.py (engine.segmentation_step, FlatAdapterOptimizer(max_norm=0) over all parameters) with
this model's checkpoint hooks; the model trains in train mode (batch statistics, dropout) and is evaluated in eval mode.  A one-channel batch
is widened on the device by the model.  Refused before anything is allocated: an img_size that is not a multiple of 16 (the reference fails in
torch.cat there).  Build additions (add_build_args): --dtype, --synthetic*, --data_pt, --stats_json, --val_every.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.models import supervised
from src.third_party.unet import UNet
from src.utils.tools import default_device


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="unet_seg")
    p.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    p.add_argument("--img_size", type=int, default=224, help="Image width and height")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction, help="Use strong augs")
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction, help="Use weak augs")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=200)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_min", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=0.01)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.95)
    p.add_argument("--device", type=str, default=default_device())
    p.add_argument("--patience", type=int, default=15, help="Early stopping patience (10 * N epochs)")
    p.add_argument("--test", default=False, action="store_true", help="Load local checkpoint for testing")
    supervised.add_build_args(p)
    return p.parse_args(argv)


def check_args(args):
    """The refusals, before any allocation."""
    if args.img_size <= 0 or args.img_size % 16:
        raise ValueError(f"--img_size {args.img_size} is not a multiple of 16: the UNet's four poolings and upsamplings would not meet its skips")


def prepare_model(args):
    check_args(args)
    torch.manual_seed(args.seed)
    return UNet(in_channels=args.in_channels, num_classes=args.num_classes).to(args.device)


def main(argv=None):
    args = get_args(argv)
    check_args(args)
    return supervised.run(args, supervised.SEGMENTATION, prepare_model)


if __name__ == "__main__":
    main()
