"""Few-shot classification data (counterpart of the reference's src/datasets/fewshot_classification.py): the classification DataModule with the
training list cut down once, before training, by one of the reference's three strategies — and with their exact results:

  * `shots_per_class` = K (overrides the ratio): names grouped by label in first-seen class order, `sample(names_c, min(K, len_c))` per class, one shuffle.
  * stratified ratio (the default): `max(1, int(len_c * ratio))` per class, one shuffle.  At ratio 1.0 this is a permutation, not the identity.
  * `stratified=False`: `sample(names, max(1, int(len * ratio)))`, one shuffle.

The draws come from a private `random.Random(args.seed)`.  The reference seeds the global `random` with args.seed in `main` and draws nothing from it
before sampling, so the stream — and every sampled list — is the same, while the global generators stay untouched here (as in src/datasets/augment.py).
Names come from the training split of `--data_pt` or `--synthetic` (src/datasets/classification.py); validation and test splits are whole.

The sampled rows do not go through a loader: `resident_rows()` hands them over as stored (a uint8 file stays uint8, channel 0; float files and the
synthetic split fp32) with their labels, and src/datasets/resident.py keeps them on the device and forms every training batch there.
"""
import os
import random
from collections import defaultdict

import torch

from src.datasets import classification as base


def check_fewshot_args(args, world=None):
    """The refusals, before anything is allocated."""
    ratio, shots = getattr(args, "train_ratio", None), getattr(args, "shots_per_class", None)
    if ratio is not None and not 0.0 < ratio <= 1.0:
        raise ValueError(f"--train_ratio {ratio} is outside (0, 1]")
    if shots is not None and shots < 1:
        raise ValueError(f"--shots_per_class {shots} is below 1")
    world = int(os.environ.get("WORLD_SIZE", 1)) if world is None else int(world)
    if world > 1:
        raise ValueError(f"few-shot runs are one process: the sampled training set lives on one device whole (world size {world})")


def sample_training_names(names, label_of, train_ratio=None, shots_per_class=None, stratified=True, rng=random):
    """The reference's FewShotDataModule._sample_training_data (:72-131) on `names`, label_of a dict name -> label (absent: 0), drawing from `rng`."""
    if shots_per_class is None and train_ratio is None:
        return names
    if shots_per_class is None and not stratified:
        sampled = rng.sample(names, max(1, int(len(names) * train_ratio)))
        rng.shuffle(sampled)
        return sampled
    by_class = defaultdict(list)
    for name in names:
        by_class[label_of.get(name, 0)].append(name)
    sampled = []
    for members in by_class.values():
        k = min(shots_per_class, len(members)) if shots_per_class is not None else max(1, int(len(members) * train_ratio))
        sampled.extend(rng.sample(members, k))
    rng.shuffle(sampled)
    return sampled


class FewShotDataModule(base.DataModule):
    def __init__(self, args, train_ratio=None, shots_per_class=None, stratified=True, rank=0, world=1):
        check_fewshot_args(args, world)
        super().__init__(args, rank=rank, world=world)
        self.train_ratio, self.shots_per_class, self.stratified = train_ratio, shots_per_class, stratified
        full = self.train_dataset
        names = list(full.names)
        if len(set(names)) != len(names):
            raise ValueError("few-shot sampling draws names: the training split's names must be distinct")
        label_of = {n: int(l) for n, l in zip(names, full.labels.tolist())}
        sampled = sample_training_names(names, label_of, train_ratio, shots_per_class, stratified, random.Random(args.seed))
        print("  Few-shot sampling:")
        print(f"    - Original training samples: {len(names)}")
        print(f"    - Sampled training samples: {len(sampled)}")
        if shots_per_class is not None:
            print(f"    - Shots per class: {shots_per_class}")
        elif train_ratio is not None:
            print(f"    - Train ratio: {train_ratio * 100:.1f}%")
        at = {n: i for i, n in enumerate(names)}
        idx = [at[n] for n in sampled]
        self.train_dataset = base.TensorClassification(full.images[idx], full.labels[idx], sampled)
        self.original_train_count, self.sampled_train_count = len(names), len(sampled)

    def resident_rows(self):
        """(images [n, 1, S, S] uint8 or fp32 as stored, labels int64 [n]) of the sampled training rows."""
        images = self.train_dataset.images[:, :1]
        images = images if images.dtype == torch.uint8 else images.float()
        return images.contiguous(), self.train_dataset.labels.to(torch.int64).contiguous()


def from_args(args, rank=0, world=1):
    """What supervised.train builds: the module from --train_ratio / --shots_per_class."""
    return FewShotDataModule(args, train_ratio=args.train_ratio, shots_per_class=getattr(args, "shots_per_class", None), rank=rank, world=world)
