"""DINOv2 ViT-B/14 + UNet decoder segmentation on the HIP path — counterpart of the reference's src/models/dino/segmentation.py.

Kept: the command line (exp dino_seg, img_size 518, patch_size 14, decoder_type unet, batch 24, 1000 epochs, patience 15, AdamW 1e-4 / betas 0.9, 0.95 /
weight decay 0.01, cosine per iteration to --lr_min, no clipping), model preparation (vit_base(img_size, patch_size) in DINOV2Encoder(n_last_blocks=5),
ckpt/dinov2_vitb14_pretrain.pth with checkpoint key "student" when it exists, the tower frozen and always in eval mode; setup_decoders(768, [lr],
num_classes, "unet", img_size, patch_size)), DiceCE per iteration, validation every 10 epochs and at the last one with best-by-Dice, early stopping
by --patience, a test pass after each validation, the checkpoint `decoders.state_dict()` (BatchNorm buffers included) loaded with strict=False by
test(), and the Dice / IoU / HD95 / ASD table with results.csv.
The loop is src/models/supervised.py (engine.segmentation_step, FlatAdapterOptimizer(max_norm=0) over the decoder parameters) with
this model's checkpoint hooks; the decoder trains in train mode and is evaluated in eval mode.  A one-channel batch goes through the tower's
channel-summed patch embedding.  Refused before anything is allocated: a decoder_type other than unet (the reference's linear decoder fails on its own
encoder output) and an img_size that is not a multiple of patch_size.  Build additions (add_build_args): --dtype, --synthetic*, --data_pt, --ckpt_path,
--stats_json, --val_every.  Without a checkpoint the tower is randomly initialised (logged).
"""
import argparse
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch
import torch.nn as nn

from src.models import supervised
from src.third_party.dino import vision_transformer as vit
from src.third_party.dino.dinov2 import DINOV2Encoder, load_pretrained_weights, setup_decoders
from src.utils.tools import default_device

DEFAULT_CKPT = "ckpt/dinov2_vitb14_pretrain.pth"


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="dino_seg")
    p.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    p.add_argument("--img_size", type=int, default=518, help="Image width and height")
    p.add_argument("--patch_size", type=int, default=14, help="Patch size")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction, help="Use strong augs")
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction, help="Use weak augs")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--decoder_type", type=str, default="unet")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=1000)
    p.add_argument("--batch_size", type=int, default=24)
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
    if args.decoder_type != "unet":
        raise ValueError(f"--decoder_type {args.decoder_type!r} is not supported: only 'unet' runs (the reference's 'linear' decoder calls .reshape on "
                         "the dict its n_last_blocks=1 encoder returns)")
    if args.img_size <= 0 or args.img_size % args.patch_size:
        raise ValueError(f"--img_size {args.img_size} is not a multiple of --patch_size {args.patch_size}: the tower has no such grid")


class DinoSegmenter(nn.Module):
    """feature_model (frozen DINOV2Encoder(n_last_blocks=5), always in eval mode) + decoders (AllDecoders holding one UNetDecoder): images -> logits
    [B, num_classes, img_size, img_size].  The checkpoint is `decoders.state_dict()`, as the reference saves it; it loads with strict=False."""

    def __init__(self, feature_model, decoders):
        super().__init__()
        self.feature_model, self.decoders = feature_model, decoders

    def train(self, mode=True):
        super().train(mode)
        self.feature_model.eval()
        return self

    def forward(self, images):
        outputs = self.decoders(self.feature_model(images))
        return outputs[next(iter(outputs))]

    def checkpoint_dict(self):
        return self.decoders.state_dict()

    def load_checkpoint(self, state):
        self.decoders.load_state_dict(state, strict=False)


def build_model(img_size=518, patch_size=14, num_classes=2, lr=1e-4, ckpt=None, depth=12, embed_dim=768, num_heads=12, decoder_type="unet"):
    """The reference's prepare_model on the CPU."""
    model = vit.DinoVisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4)
    feature_model = DINOV2Encoder(model, n_last_blocks=5)
    if ckpt is not None:
        load_pretrained_weights(feature_model, ckpt, "student")
    for param in feature_model.parameters():
        param.requires_grad = False
    decoders, _ = setup_decoders(embed_dim, [lr], num_classes=num_classes, decoder_type=decoder_type, image_size=img_size, patch_size=patch_size)
    return DinoSegmenter(feature_model, decoders)


def prepare_model(args):
    check_args(args)
    ckpt = args.ckpt_path or (DEFAULT_CKPT if os.path.exists(DEFAULT_CKPT) else None)
    if ckpt is None:
        logging.info(f"no DINOv2 checkpoint ({DEFAULT_CKPT} absent, no --ckpt_path): the tower is randomly initialised")
    torch.manual_seed(args.seed)
    return build_model(args.img_size, args.patch_size, args.num_classes, args.lr, ckpt).to(args.device)


def main(argv=None):
    args = get_args(argv)
    check_args(args)
    return supervised.run(args, supervised.SEGMENTATION, prepare_model)


if __name__ == "__main__":
    main()
