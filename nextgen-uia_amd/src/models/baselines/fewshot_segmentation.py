"""The UNet few-shot segmentation baseline on the HIP path — counterpart of the reference's src/models/baselines/fewshot_segmentation.py: the
data-efficiency runs of the paper's tables (Baseline, LoRA and Mona at 1 %, 5 % and 10 % of the training list).

It is src/models/baselines/segmentation.py on a training list sampled once: the same `prepare_model` (UNet(in_channels, num_classes), every parameter
trainable), the same loop (src/models/supervised.py: criterion, AdamW with a per-iteration cosine schedule, validation schedule, best checkpoint,
--patience, the test pass after each validation), the same checkpoint dict, result table and backup folder; `test()` evaluates the whole test split
with the plain DataModule. Kept from the reference: its flags and defaults, --train_ratio, --exp fewshot_unet_seg, the three "Few-shot sampling" lines
and `Training samples: a / b`.  The reference's README calls these entries with `--ratio`, a flag they do not define; the flag is --train_ratio.

Different on purpose: the sampled training set lives on the device whole and every training batch is formed there by one launch
(src/datasets/resident.py, uia_augment_gather): B = min(batch_size, n), drop_last = n > batch_size, a fresh permutation per epoch, --strong_augs /
--weak_augs run by the same launch on --data_pt rows.  train()'s dict and --stats_json carry original_train_count / sampled_train_count.  One process:
refused under torch.distributed.run with a world size above 1.  B = 1 runs: the BatchNorm kernels (csrc/unet_bn.hip) take any population M = B H W >=
1 (DESIGN.md §4 "Few-shot").
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

from src.datasets.fewshot_classification import check_fewshot_args
from src.models import supervised
from src.models.baselines import segmentation as supervised_entry
from src.utils.tools import default_device

TASK = supervised.FEWSHOT_SEGMENTATION
prepare_model = supervised_entry.prepare_model                  # the supervised entry's model: UNet(in_channels, num_classes), every parameter trainable


def get_args(argv=None):
    p = argparse.ArgumentParser("Few-shot Segmentation with UNet")
    p.add_argument("--exp", type=str, default="fewshot_unet_seg")
    p.add_argument("--dataset", type=str, default="LN-INT", help="Dataset name")
    p.add_argument("--img_size", type=int, default=224, help="Image width and height")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--train_ratio", type=float, default=0.1, help="Percentage of training data to use (0.0-1.0)")
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
    """The refusals, before anything is allocated."""
    check_fewshot_args(args)
    supervised_entry.check_args(args)


def train(args, prepare=None):
    check_args(args)
    return supervised.train(args, TASK, prepare or prepare_model)


def test(args, prepare=None):
    """The whole test split through the plain DataModule, as the reference's test()."""
    return supervised.test(args, TASK, prepare or prepare_model)


def main(argv=None):
    args = get_args(argv)
    check_args(args)
    return supervised.run(args, TASK, prepare_model)


if __name__ == "__main__":
    main()
