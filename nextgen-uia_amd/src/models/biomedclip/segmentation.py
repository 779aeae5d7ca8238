"""BiomedCLIP segmentation with the feature-pyramid adapter on the HIP path — counterpart of the reference's
src/models/biomedclip/segmentation.py.  The loop is src/models/supervised.py with its SEGMENTATION task; `train` / `test` here delegate to it.

Kept: the command line (:28-72; default --mona_variant hybrid, batch 32, AdamW betas 0.9/0.95, no gradient clipping), model
assembly (:81-135: optional LoRA or Mona adapters loaded BY NAME from a fine-tune checkpoint, TimmCLIPAdapter(task="seg") on
layers 3/6/9, freeze_clip_backbone()), the loop (:138-255): DiceCE(to_onehot_y, softmax, squared_pred) per iteration with a
per-iteration cosine schedule, validation by mean foreground Dice every 10 epochs and at the last one, early stopping by
--patience, and the checkpoint dict {"reduces", "blocks", "seg_head", "mona"} (:212-225) under runs/<exp>/<dataset>/train.
the test pass after every validation (:259-280), `test()` (:283-355: checkpoint -> heads + Mona parameters by name -> metrics over the test split -> the
Metric / Mean / Std table, results.csv and the backup folder) and `main` (train unless --test, then ALWAYS test).
Different on purpose: the iteration is engine.segmentation_step with nothing read on the host, batches through engine.DevicePrefetcher (one grayscale channel +
a uint8 mask per image, repeated on the device), --strong_augs / --weak_augs applied to --data_pt training batches on the device (src/datasets/augment.py),
Dice / IoU and, for two-class logits, MONAI's HD95 / ASD on the device (uia_surface_distances), the test pass's visualize_seg pictures (three PNG
files per test image under <test dir>/viz) from one launch per batch behind the metrics with background writers (src/utils/viz.py; --no-viz: none) and
TensorBoard scalars go to <train dir>/log/scalars.jsonl.  Data: `--synthetic` or `--data_pt` (src/datasets/segmentation.py).
"""
import argparse
import logging
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.adapters import inject_lora_to_biomedclip, inject_mona_variant_to_open_clip
from src.adapters.checkpoint import load_adapter_by_name
from src.models import supervised
from src.third_party.biomedclip.model import create_biomedclip
from src.third_party.timm.clip_adapter import TimmCLIPAdapter
from src.utils.tools import default_device, parse_config


def get_args(argv=None):
    p = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    p.add_argument("--exp", type=str, default="biomedclip_seg")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction)
    p.add_argument("--mona_variant", type=str, default="hybrid")
    p.add_argument("--mona_weights", type=str, default=None)
    p.add_argument("--in_channels", type=int, default=3)
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--reduce_dim", type=int, default=512)
    p.add_argument("--mona_bottleneck", type=int, default=64)
    p.add_argument("--mona_layers", type=int, default=None)
    p.add_argument("--lora_weights", type=str, default=None)
    p.add_argument("--lora_r", type=int, default=16)
    p.add_argument("--lora_alpha", type=int, default=32)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--epochs", type=int, default=200)
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


criterion = supervised.SEGMENTATION.criterion                   # reference :76: DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)


def prepare_model(args):
    cfg = parse_config(args.model_config) if args.model_config else None
    state = torch.load(args.ckpt_path, map_location="cpu") if args.ckpt_path else None
    clip_model = create_biomedclip(state_dict=state, config=cfg, seed=args.seed)
    clip_model.float()
    if args.lora_weights:
        inject_lora_to_biomedclip(clip_model, lora_r=args.lora_r, lora_alpha=args.lora_alpha, lora_dropout=0.0)
        n = load_adapter_by_name(clip_model, args.lora_weights, "lora_state_dict")
        logging.info(f"✓ Loaded {n} pretrained LoRA parameters from {args.lora_weights}")
    elif args.mona_weights:
        inject_mona_variant_to_open_clip(clip_model, variant=args.mona_variant, bottleneck_dim=args.mona_bottleneck, num_layers=args.mona_layers)
        n = load_adapter_by_name(clip_model, args.mona_weights, "mona_state_dict")
        logging.info(f"✓ Loaded {n} pretrained MONA parameters from {args.mona_weights}")
    adapter = TimmCLIPAdapter(clip_model=clip_model, extract_layers=supervised.extract_layers(args), reduce_dim=args.reduce_dim,
                              num_classes=args.num_classes, img_size=args.img_size, patch_size=args.patch_size, task="seg")
    adapter.to(args.device)
    adapter.freeze_clip_backbone()
    return adapter


def train(args, prepare=None):
    """prepare: args -> model (default: this entry point's prepare_model)."""
    return supervised.train(args, supervised.SEGMENTATION, prepare or prepare_model)


def test(args, prepare=None):
    """reference :283-355."""
    return supervised.test(args, supervised.SEGMENTATION, prepare or prepare_model)


def main(argv=None):
    return supervised.run(get_args(argv), supervised.SEGMENTATION, prepare_model)


if __name__ == "__main__":
    main()
