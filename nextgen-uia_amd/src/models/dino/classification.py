"""DINOv2 ViT-B/14 linear classification on the HIP path — counterpart of the reference's src/models/dino/classification.py.

Kept: the command line (:29-63: exp dino_cls, img_size 518, patch_size 14, batch 24, 1000 epochs, patience 15, AdamW 1e-4 / betas 0.9, 0.95 /
weight decay 0.01, cosine to --lr_min), model preparation (:66-87: vit_base(img_size, patch_size) wrapped in DINOV2Encoder(n_last_blocks=4),
ckpt/dinov2_vitb14_pretrain.pth loaded through load_pretrained_weights with checkpoint key "student" when the file exists, the backbone frozen in
eval mode; ClassificationHead(768, num_classes, layers=4)), and the loop (:90-235): FocalLoss(to_onehot_y=True), AdamW over the classifier only,
validation at `epoch > 0 and epoch % 10 == 0` and at the last epoch, best-by-accuracy `classifier.state_dict()` in best_model.pth, early stopping by
--patience, a test-split pass after every validation, and test() with the Acc / Rec / Pre / F1 / AUC table, results.csv and the backup folder.
The loop is src/models/supervised.py with this model's checkpoint hooks.
Build additions (add_build_args): --dtype, --synthetic*, --data_pt, --ckpt_path (a DINOv2 checkpoint in place of the default path), --stats_json,
--val_every.  Without a checkpoint the tower is randomly initialised (logged).
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
from src.third_party.dino.dinov2 import ClassificationHead, DINOV2Encoder, load_pretrained_weights
from src.utils.tools import default_device

DEFAULT_CKPT = "ckpt/dinov2_vitb14_pretrain.pth"


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="dino_cls")
    p.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    p.add_argument("--img_size", type=int, default=518, help="Image width and height")
    p.add_argument("--patch_size", type=int, default=14, help="Patch size")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction, help="Use strong augs")
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction, help="Use weak augs")
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
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


class DinoClassifier(nn.Module):
    """feature_model (frozen DINOV2Encoder, always in eval mode) + classifier (ClassificationHead): images -> logits.  The checkpoint is the
    classifier's state dict alone ({"linear.weight", "linear.bias"}), as the reference saves it."""

    def __init__(self, feature_model, classifier):
        super().__init__()
        self.feature_model, self.classifier = feature_model, classifier

    def train(self, mode=True):
        super().train(mode)
        self.feature_model.eval()                                   # reference :93: the backbone stays in eval mode
        return self

    def forward(self, images):
        return self.classifier(self.feature_model(images))

    def checkpoint_dict(self):
        return self.classifier.state_dict()

    def load_checkpoint(self, state):
        self.classifier.load_state_dict(state)


def build_model(img_size=518, patch_size=14, num_classes=2, ckpt=None, depth=12, embed_dim=768, num_heads=12, n_last_blocks=4):
    """The reference's prepare_model (:66-87) on the CPU: returns the frozen DinoClassifier (the head trainable)."""
    model = vit.DinoVisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4)
    feature_model = DINOV2Encoder(model, n_last_blocks=n_last_blocks)
    if ckpt is not None:
        load_pretrained_weights(feature_model, ckpt, "student")
    for param in feature_model.parameters():
        param.requires_grad = False
    classifier = ClassificationHead(embed_dim=embed_dim, num_classes=num_classes, layers=n_last_blocks)
    return DinoClassifier(feature_model, classifier)


def prepare_model(args):
    ckpt = args.ckpt_path or (DEFAULT_CKPT if os.path.exists(DEFAULT_CKPT) else None)
    if ckpt is None:
        logging.info(f"no DINOv2 checkpoint ({DEFAULT_CKPT} absent, no --ckpt_path): the tower is randomly initialised")
    torch.manual_seed(args.seed)
    model = build_model(args.img_size, args.patch_size, args.num_classes, ckpt)
    return model.to(args.device)


def main(argv=None):
    return supervised.run(get_args(argv), supervised.CLASSIFICATION, prepare_model)


if __name__ == "__main__":
    main()
