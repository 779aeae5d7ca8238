"""Few-shot segmentation data (counterpart of the reference's src/datasets/fewshot_segmentation.py): the segmentation DataModule with the training
list cut down once, before training, exactly as the reference cuts it: `train_ratio < 1.0` gives `sample(names, max(1, int(len * ratio)))` and one
shuffle; `train_ratio >= 1.0` (or None) leaves the list untouched.

The draws come from a private `random.Random(args.seed)`: the reference seeds the global `random` with args.seed in `main` and draws nothing from it
before sampling, so the sampled list is the same and the global generators stay untouched (as in src/datasets/augment.py).  Names come from the
training split of `--data_pt` or `--synthetic` (src/datasets/segmentation.py); validation and test splits are whole.

The sampled rows do not go through a loader: `resident_rows()` hands them over as stored (a uint8 file stays uint8, channel 0; float files and the
synthetic split fp32) with their masks as bytes, and src/datasets/resident.py keeps them on the device and forms every training batch there.
"""
import random

import torch

from src.datasets import segmentation as base
from src.datasets.fewshot_classification import check_fewshot_args


def sample_training_names(names, train_ratio=None, rng=random):
    """The reference's FewShotDataModule._sample_training_data (:56-65) on `names`, drawing from `rng`."""
    if train_ratio is not None and train_ratio < 1.0:
        sampled = rng.sample(names, max(1, int(len(names) * train_ratio)))
        rng.shuffle(sampled)
        return sampled
    return names


class _Rows(torch.utils.data.Dataset):
    """The rows `idx` of a dataset that makes its samples on access (the synthetic split)."""

    def __init__(self, ds, idx):
        self.ds, self.idx = ds, list(idx)

    def __len__(self):
        return len(self.idx)

    def name_of(self, i):
        return self.ds.name_of(self.idx[i])

    def __getitem__(self, i):
        return self.ds[self.idx[i]]


class FewShotDataModule(base.DataModule):
    def __init__(self, args, train_ratio=None, rank=0, world=1):
        check_fewshot_args(args, world)
        super().__init__(args, rank=rank, world=world)
        self.train_ratio = train_ratio
        full = self.train_dataset
        names = [full.name_of(i) for i in range(len(full))]
        if len(set(names)) != len(names):
            raise ValueError("few-shot sampling draws names: the training split's names must be distinct")
        sampled = sample_training_names(names, train_ratio, random.Random(args.seed))
        print("  Few-shot sampling:")
        print(f"    - Original training samples: {len(names)}")
        print(f"    - Sampled training samples: {len(sampled)}")
        if train_ratio is not None:
            print(f"    - Train ratio: {train_ratio * 100:.1f}%")
        at = {n: i for i, n in enumerate(names)}
        idx = [at[n] for n in sampled]
        if isinstance(full, base.TensorSegmentation):
            self.train_dataset = base.TensorSegmentation(full.images[idx], full.labels[idx], sampled)
        else:
            self.train_dataset = _Rows(full, idx)
        self.original_train_count, self.sampled_train_count = len(names), len(sampled)

    def resident_rows(self):
        """(images [n, 1, S, S] uint8 or fp32 as stored, masks uint8 [n, 1, S, S] in {0, 1}) of the sampled training rows."""
        ds = self.train_dataset
        if isinstance(ds, base.TensorSegmentation):
            images = ds.images[:, :1]
            images = images if images.dtype == torch.uint8 else images.float()
            return images.contiguous(), (ds.labels[:, :1] > 0).to(torch.uint8).contiguous()
        rows = [ds[i] for i in range(len(ds))]
        return torch.stack([r[0] for r in rows]).contiguous(), torch.stack([r[1] for r in rows]).contiguous()


def from_args(args, rank=0, world=1):
    """What supervised.train builds: the module from --train_ratio."""
    return FewShotDataModule(args, train_ratio=args.train_ratio, rank=rank, world=world)
