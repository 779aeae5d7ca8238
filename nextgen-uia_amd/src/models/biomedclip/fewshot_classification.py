"""BiomedCLIP few-shot classification on the HIP path — counterpart of the reference's src/models/biomedclip/fewshot_classification.py: the
data-efficiency runs of the paper's tables (Baseline, LoRA and Mona at 1 %, 5 % and 10 % of the training list, or at K shots per class).

It is src/models/biomedclip/classification.py on a training list sampled once: the same `prepare_model` (optional LoRA or Mona adapters loaded by
name, TimmCLIPAdapter(task="cls"), freeze_clip_backbone()), the same loop (src/models/supervised.py: criterion, AdamW with a per-iteration cosine
schedule, validation schedule, best checkpoint, --patience, the test pass after each validation), the same checkpoint dict, result table and backup
folder; `test()` evaluates the whole test split with the plain DataModule. Kept from the reference: its flags and defaults, --train_ratio /
--shots_per_class, --exp fewshot_cls, the three "Few-shot sampling" lines and `Training samples: a / b`, and the data of plot_roc_curve after each
validation as roc_curves/roc_curve_iter_<iter>.csv under the train directory (no figure).  The reference's README calls these entries with `--ratio`,
a flag they do not define; the flag is --train_ratio.

Different on purpose: the sampled training set lives on the device whole and every training batch is formed there by one launch
(src/datasets/resident.py, uia_augment_gather): B = min(batch_size, n), drop_last = n > batch_size, a fresh permutation per epoch, --strong_augs /
--weak_augs run by the same launch on --data_pt rows.  train()'s dict and --stats_json carry original_train_count / sampled_train_count.  One process:
refused under torch.distributed.run with a world size above 1.  Runs at n = 1 (B = 1): nothing in the model normalises over the batch.
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[3]))

from src.datasets.fewshot_classification import check_fewshot_args
from src.models import supervised
from src.models.biomedclip import classification as supervised_entry
from src.utils.tools import default_device

TASK = supervised.FEWSHOT_CLASSIFICATION
prepare_model = supervised_entry.prepare_model                  # the supervised entry's model: optional LoRA or Mona adapters loaded by name, TimmCLIPAdapter(task="cls"), freeze_clip_backbone()


def get_args(argv=None):
    p = argparse.ArgumentParser("Few-shot Classification with BiomedCLIP")
    p.add_argument("--exp", type=str, default="fewshot_cls")
    p.add_argument("--dataset", type=str, default="LN-INT")
    p.add_argument("--img_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--train_ratio", type=float, default=0.1, help="Percentage of training data to use (0.0-1.0)")
    p.add_argument("--shots_per_class", type=int, default=None, help="Number of samples per class (overrides train_ratio)")
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


def check_args(args):
    """The refusals, before anything is allocated."""
    check_fewshot_args(args)


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
