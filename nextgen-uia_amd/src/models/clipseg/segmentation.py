"""CLIPSeg segmentation on the HIP path — drop-in for the reference's src/models/clipseg/segmentation.py (BASELINE configs[3]).

Kept, by reference line:
  :28-66    every flag with its default (--dataset LN-INT, --epochs 1000, --lr_min 1e-8, --beta1 0.9 / --beta2 0.95, --patience 15, --strong_augs / --weak_augs
            as BooleanOptionalAction, --version, --ckpt, --patch_size, --test ...)
  :69-82    get_prompt: LN-INT / LN-EXT -> ln_prompt, BUSI -> busi_prompt, DDTI / TN3K -> thyroid_prompt, Prostate -> prostate_prompt, anything else None
  :85       DiceCELoss(to_onehot_y, softmax, squared_pred, smooth 1e-8 / 1e-8), a module-level `criterion`
  :88-105   prepare_model: CLIP from --ckpt in fp32 -> CLIPSegAdapter -> freeze_clip_backbone()
  :108-236  train: AdamW(decoder, lr, betas, weight_decay), CosineAnnealingLR over len(trainloader) * epochs ITERATIONS stepped per iteration, the fixed prompt
            repeated over the batch (:142), validation when (epoch > 0 and epoch % 10 == 0) or at the last epoch -> MetricAccumulator -> best mean Dice ->
            {"decoder": state_dict} in runs/<exp>/<dataset>/train/best_model.pth (:190-197), else patience += 1, early stop at --patience (:201-204), then the
            same pass over the test split (:212-231)
  :238-308  test: best_model.pth -> decoder, metrics over the test split, a Metric / Mean / Std table logged and written to
            runs/<exp>/<dataset>/test/<time>_iou=<iou>/results.csv beside copies of the checkpoint and the log
  :311-341  main: seeds, the two run directories, train unless --test, then ALWAYS test.

Different on purpose: the iteration is engine.segmentation_step — the step `bench.py --config clipseg` times — and nothing is read on the host per iteration
(the reference's loss.item() every tenth iteration goes to a log of device scalars that is flushed at validation time); batches arrive through
engine.DevicePrefetcher (loader workers -> shared-memory ring -> copy stream), one grayscale channel + a uint8 mask per image, repeated to three channels on the
device; --strong_augs / --weak_augs act on --data_pt training batches there too (src/datasets/augment.py, one launch per batch); validation metrics are
computed on the device (Dice / IoU, MONAI semantics; HD95 / ASD are host-side scipy work and are reported as NaN); TensorBoard scalars go to <train dir>/log/scalars.jsonl.  Data: --synthetic or --data_pt (src/datasets/segmentation.py).  Build-only flags are listed after the
reference's in get_args.  Data parallel under torch.distributed.run: every rank trains on its shard, ONE all-reduce of the decoder gradients per iteration.
"""
import argparse
import dataclasses
import logging
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

import torch

from src.datasets import folder as dataset_folder
from src.datasets.segmentation import synthetic_batch      # noqa: F401  (bench.py and tools import it from here)
from src.models import supervised
from src.models.clipseg.prompt import busi_prompt, ln_prompt, prostate_prompt, thyroid_prompt
from src.third_party.openai_clip.clipseg_adapter import CLIPSegAdapter
from src.third_party.openai_clip.model import CLIP, build_model
from src.utils.tools import default_device

# The loop is src/models/supervised.py; beside the segmentation task's fields this entry logs the lr scalar and the HD95 / ASD scalars, times the loop's
# host side per epoch (bench.py prints the records) and repeats the reference's early-stopping line (:201-204).
TASK = dataclasses.replace(supervised.SEGMENTATION, scalars=("loss", "dice_mean", "iou_mean", "hd95_mean", "asd_mean"), lr_scalar=True, loop_timings=True,
                           stop_twice=True)


def get_args(argv=None):
    """Get arguments from command line (reference :28-66, then this build's additions)."""
    parser = argparse.ArgumentParser("Adaptation of Visual Foundation Model for Medical Ultrasound Image Analysis")
    # Data related
    parser.add_argument("--exp", type=str, default="clipseg")
    parser.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    parser.add_argument("--img_size", type=int, default=224, help="Image width and height")
    parser.add_argument("--patch_size", type=int, default=16, help="Patch size")
    parser.add_argument("--num_workers", type=int, default=8)
    # Augmentation related (applied to --data_pt training batches on the device: src/datasets/augment.py)
    parser.add_argument("--strong_augs", default=True, action=argparse.BooleanOptionalAction, help="Use strong augs")
    parser.add_argument("--weak_augs", default=True, action=argparse.BooleanOptionalAction, help="Use weak augs")
    # Model related
    parser.add_argument("--version", type=str, default="ViT-B/16")
    parser.add_argument("--ckpt", type=str, default="ckpt/ViT-B-16.pt")
    parser.add_argument("--in_channels", type=int, default=3)
    parser.add_argument("--num_classes", type=int, default=2)
    parser.add_argument("--reduce_dim", type=int, default=512)           # unused by the reference as well (the decoder's own 64 applies)
    # Training related
    parser.add_argument("--seed", type=int, default=1)
    parser.add_argument("--epochs", type=int, default=1000)
    parser.add_argument("--batch_size", type=int, default=32)
    parser.add_argument("--lr", type=float, default=1e-4)
    parser.add_argument("--lr_min", type=float, default=1e-8)
    parser.add_argument("--weight_decay", type=float, default=0.01)
    parser.add_argument("--beta1", type=float, default=0.9)
    parser.add_argument("--beta2", type=float, default=0.95)
    parser.add_argument("--device", type=str, default=default_device())
    parser.add_argument("--patience", type=int, default=15, help="Early stopping patience (10 * N epochs)")
    # Testing related
    parser.add_argument("--test", default=False, action="store_true", help="Load local checkpoint for testing")
    # ---- additions of this build (none changes a reference default)
    parser.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="operand precision of the HIP kernels (masters stay fp32)")
    parser.add_argument("--synthetic", action="store_true", help="synthetic images + ellipse masks instead of ../data/NextGen-UIA")
    parser.add_argument("--synthetic_train", type=int, default=256)
    parser.add_argument("--synthetic_val", type=int, default=64)
    parser.add_argument("--synthetic_test", type=int, default=64)
    parser.add_argument("--data_pt", type=str, default=None, help=".pt file {images, labels[, names, split]} (src/datasets/segmentation.py)")
    parser.add_argument("--decoder_ckpt", type=str, default=None, help="CIDAS/clipseg-rd64-refined decoder state dict (the reference downloads it)")
    parser.add_argument("--val_every", type=int, default=10, help="epochs between validations (reference: fixed 10)")
    parser.add_argument("--stats_json", type=str, default=None, help="write per-epoch timings / counters of the training loop here")
    parser.add_argument("--viz", default=True, action=argparse.BooleanOptionalAction,
                        help="test(): write <stem>.png / <stem>_overlay.png / <stem>_pred.png per test image (reference: always)")
    return parser.parse_args(argv)


def get_prompt(args):
    """Get tokenized prompt according to the dataset (reference :69-82)."""
    prompt = None
    if args.dataset == "LN-INT" or args.dataset == "LN-EXT":
        prompt = ln_prompt
    elif args.dataset == "BUSI":
        prompt = busi_prompt
    elif args.dataset == "DDTI" or args.dataset == "TN3K":
        prompt = thyroid_prompt
    elif args.dataset == "Prostate":
        prompt = prostate_prompt
    return prompt


# Loss function (reference :85): DiceCELoss(smooth_nr=1e-8, smooth_dr=1e-8)
criterion = TASK.criterion

_GEOMETRY = {   # random-init geometry per --version when --synthetic runs without a checkpoint: (embed, layers, width, patch, text width, text heads)
    "ViT-B/32": (512, 12, 768, 32, 512, 8), "ViT-B/16": (512, 12, 768, 16, 512, 8), "ViT-L/14": (768, 24, 1024, 14, 768, 12),
}


def load_clip(args):
    """clip.load(args.ckpt) of the reference (:90; clip.py:97-150 accepts a TorchScript archive or a plain state dict)."""
    if args.ckpt and os.path.exists(args.ckpt):
        try:
            state = torch.jit.load(args.ckpt, map_location="cpu").state_dict()
        except RuntimeError:
            state = torch.load(args.ckpt, map_location="cpu")
            state = state.get("state_dict", state) if isinstance(state, dict) else state.state_dict()
        return build_model(state)
    if not args.synthetic:
        raise FileNotFoundError(f"Model {args.ckpt} not found (download the OpenAI {args.version} checkpoint, or pass --synthetic for randomly initialised weights)")
    if args.version not in _GEOMETRY:
        raise NotImplementedError(f"--version {args.version}: only ViT variants run on this path ({', '.join(_GEOMETRY)})")
    e, layers, width, patch, tw, th = _GEOMETRY[args.version]
    logging.info(f"{args.ckpt} not found: randomly initialised {args.version} (--synthetic)")
    torch.manual_seed(args.seed)
    return CLIP(e, args.img_size, layers, width, patch, 77, 49408, tw, th, 12)


def prepare_model(args):
    clip_model = load_clip(args)
    clip_model.float()                                           # reference :92-95
    adapter = CLIPSegAdapter(clip_model=clip_model)
    if args.decoder_ckpt:
        adapter.decoder.load_state_dict(torch.load(args.decoder_ckpt, map_location="cpu"))
    adapter.to(args.device)
    adapter.freeze_clip_backbone()
    return adapter


def check_args(args):
    """The refusals, before any allocation."""
    dataset_folder.refuse(args, "the CLIPSeg loop")
    if get_prompt(args) is None:
        raise ValueError(f"no prompt for --dataset {args.dataset} (LN-INT, LN-EXT, BUSI, DDTI, TN3K, Prostate; reference get_prompt returns None and fails at .repeat)")


def _batch_prompt(args):
    """-> batch size -> {"input_ids": prompt.repeat(n, 1)} (:142), ONE tensor object per batch size: CLIPSegAdapter recognises an unchanged prompt tensor
    without looking at its contents."""
    prompt = get_prompt(args).to(args.device)
    cache = {}

    def kwargs_for(n):
        if n not in cache:
            cache[n] = {"input_ids": prompt.repeat(n, 1)}
        return cache[n]
    return kwargs_for


def train(args):
    check_args(args)
    return supervised.train(args, TASK, prepare_model, _batch_prompt)


def test(args):
    check_args(args)
    return supervised.test(args, TASK, prepare_model, _batch_prompt)


def main(argv=None):
    args = get_args(argv)
    check_args(args)
    out = supervised.run(args, TASK, prepare_model, _batch_prompt)
    test_stats = out.pop("test")
    return {"test": test_stats} if args.test else {"train": out, "test": test_stats}


if __name__ == "__main__":
    main()
