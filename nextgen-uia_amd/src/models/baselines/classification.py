"""The ResNet classification baseline on the HIP path — counterpart of the reference's src/models/baselines/classification.py (step 1 of
scripts/baselines.sh, the yardstick of the paper's classification tables).

Kept: the command line (exp resnet_cls, --version resnet18, img_size 224, batch 32, 200 epochs, patience 15, AdamW 1e-4 / betas 0.9, 0.95 /
weight decay 0.01, cosine per iteration to --lr_min), prepare_model = the torchvision-named ResNet with `fc` replaced by
Linear(512, num_classes) and every parameter trainable, FocalLoss(to_onehot_y=True) per iteration, validation every 10 epochs and at the last
one with best-by-accuracy, early stopping by --patience, a test pass after each validation, the checkpoint `model.state_dict()` (BatchNorm
buffers included) under runs/<exp>/<dataset>/train, and the Acc / Rec / Pre / F1 / AUC table with results.csv under runs/<exp>/<dataset>/test.
The loop is the BiomedCLIP classification entry point's (engine.segmentation_step, FlatAdapterOptimizer(max_norm=0) over all parameters) with
this model's checkpoint hooks; the model trains in train mode (batch statistics) and is evaluated in eval mode.

Different on purpose: the reference starts from torchvision's ImageNet weights, downloaded at run time.  Here --ckpt_path names a torchvision
state dict on disk (its fc.* are dropped when their shape is not num_classes', as the reference replaces fc); without it the model starts
from torchvision's random initialisation and says so once.  --version resnet50 / resnet101 / resnet152 (Bottleneck) are not built and, like an
--img_size below 32, are refused before anything is allocated.  Build additions (add_build_args): --dtype, --synthetic*, --data_pt,
--stats_json, --ckpt_path, --val_every.
"""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.models import supervised
from src.third_party import resnet
from src.utils.tools import default_device


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="resnet_cls")
    p.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    p.add_argument("--img_size", type=int, default=224, help="Image width and height")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction, help="Use strong augs")
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction, help="Use weak augs")
    p.add_argument("--version", type=str, default="resnet18")
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
    if args.version in resnet.NOT_BUILT:
        raise ValueError(f"--version {args.version} is not built: the Bottleneck ResNets ({', '.join(resnet.NOT_BUILT)}) have no HIP path here; "
                         f"built: {', '.join(resnet.BUILT)}")
    if args.version not in resnet.BUILT:
        raise ValueError(f"Invalid model version: {args.version}")
    if args.img_size < resnet.MIN_SIDE:
        raise ValueError(f"--img_size {args.img_size} is below {resnet.MIN_SIDE}: the ResNet's five halvings leave no pixel to pool")


_SAID = set()


def prepare_model(args):
    check_args(args)
    torch.manual_seed(args.seed)
    model = resnet.ResNet(resnet.BasicBlock, resnet.BUILT[args.version], num_classes=args.num_classes)
    if args.ckpt_path:
        dropped = model.load_torchvision(torch.load(args.ckpt_path, map_location="cpu"))
        logging.info(f"✓ Loaded {args.version} weights from {args.ckpt_path}" + (f" (dropped {', '.join(dropped)}: not [{args.num_classes}])" if dropped else ""))
    elif "init" not in _SAID:
        _SAID.add("init")
        logging.info(f"{args.version} starts from torchvision's random initialisation: the reference starts from the ImageNet weights, which it "
                     "downloads at run time; pass a torchvision state dict with --ckpt_path to start from them")
    return model.to(args.device)


def main(argv=None):
    args = get_args(argv)
    check_args(args)
    return supervised.run(args, supervised.CLASSIFICATION, prepare_model)


if __name__ == "__main__":
    main()
