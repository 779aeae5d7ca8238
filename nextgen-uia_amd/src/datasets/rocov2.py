"""Image / caption pairs for the retrieval entry point — the module the reference's src/models/biomedclip/retrieval.py imports (:14) and uses
(:315-323, :194) but never shipped: `ROCOv2DataModule(args, cache_dir=..., max_samples=..., seed=...)` with `train_dataloader(shuffle=False)`,
`val_dataloader()` and `test_dataloader()`, whose batches are `(images float32 [B, 3, S, S], captions list[str], ids list[str])`.

Downloading and decoding the Hugging Face ROCOv2 dataset is host I/O outside the hot path (and absent from the build image; `cache_dir` is accepted and
unused).  Data comes from
  * `--synthetic`: `args.synthetic_test` pairs per split, deterministic by `seed` (train seed, validation seed + 1, test seed + 2).  An image is one
    U[0, 1) grayscale channel repeated three times (radiology images are grayscale); a caption is a few words of a fixed vocabulary.  Every eighth
    caption repeats the one four places before it: ROCOv2 has many duplicate captions, and duplicates are what makes ties in retrieval;
  * `--data_pt`: a .pt file of {"images": uint8 or float [N, 1 or 3, S, S], "captions": list[str], optional "ids": list[str], optional "split":
    {"train": idx, "validation": idx, "test": idx}} — without "split", 70 / 10 / 20 in file order.
`max_samples` truncates every split.  A split lives in memory as tensors; loading runs in this process."""
import torch
from torch.utils.data import DataLoader, Dataset

WORDS = ("ct", "mri", "xray", "ultrasound", "axial", "sagittal", "coronal", "chest", "abdomen", "brain", "pelvis", "lesion", "mass", "nodule", "fracture",
         "effusion", "normal", "left", "right", "contrast", "enhanced", "showing", "with", "of", "the", "lobe", "liver", "kidney", "lung", "heart", "arrow", "cyst")


def synthetic_pairs(n, size, seed):
    """(images float32 [n, 1, S, S] in [0, 1), captions list[str] of n): deterministic by seed; caption i with i % 8 == 7 repeats caption i - 4."""
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(n, 1, size, size, generator=g)
    lengths = torch.randint(4, 12, (n,), generator=g).tolist()
    picks = torch.randint(0, len(WORDS), (n, 12), generator=g).tolist()
    captions = [" ".join(WORDS[w] for w in picks[i][:lengths[i]]) for i in range(n)]
    for i in range(7, n, 8):
        captions[i] = captions[i - 4]
    return images, captions


class PairDataset(Dataset):
    def __init__(self, images, captions, ids):
        assert len(images) == len(captions) == len(ids), (len(images), len(captions), len(ids))
        self.images, self.captions, self.ids = images, captions, ids

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, i):
        img = self.images[i]
        img = img.float() / 255.0 if img.dtype == torch.uint8 else img.float()
        return (img.expand(3, -1, -1) if img.shape[0] == 1 else img), self.captions[i], self.ids[i]


def _collate(samples):
    return torch.stack([s[0] for s in samples]), [s[1] for s in samples], [s[2] for s in samples]


class ROCOv2DataModule:
    SPLITS = ("train", "validation", "test")

    def __init__(self, args, cache_dir=None, max_samples=None, seed=42):
        self.args, self.cache_dir, self.max_samples, self.seed = args, cache_dir, max_samples, seed
        if getattr(args, "data_pt", None):
            blob = torch.load(args.data_pt)
            images, captions = blob["images"], list(blob["captions"])
            n = len(captions)
            ids = list(blob.get("ids") or [f"ROCOv2_{i:06d}" for i in range(n)])
            split = blob.get("split")
            if split is None:
                a, b = int(n * 0.7), int(n * 0.8)
                split = {"train": list(range(a)), "validation": list(range(a, b)), "test": list(range(b, n))}
            mk = lambda idx: PairDataset(images[list(idx)], [captions[i] for i in idx], [ids[i] for i in idx])
            sets = {s: mk(self._cut(list(split[s]))) for s in self.SPLITS}
        elif getattr(args, "synthetic", False):
            keep = self._cut(list(range(args.synthetic_test)))
            sets = {}
            for off, s in enumerate(self.SPLITS):
                images, captions = synthetic_pairs(args.synthetic_test, args.img_size, seed + off)
                sets[s] = PairDataset(images[keep], [captions[i] for i in keep], [f"ROCOv2_{s}_{i:06d}" for i in keep])
        else:
            raise RuntimeError("no dataset: pass --synthetic or --data_pt (loading the Hugging Face ROCOv2 dataset is host I/O outside this build)")
        self.train_dataset, self.val_dataset, self.test_dataset = sets["train"], sets["validation"], sets["test"]

    def _cut(self, idx):
        return idx if self.max_samples is None else idx[:self.max_samples]

    def _loader(self, ds, shuffle=False):
        g = torch.Generator().manual_seed(self.seed) if shuffle else None
        return DataLoader(ds, batch_size=self.args.batch_size, shuffle=shuffle, drop_last=False, num_workers=0, collate_fn=_collate, generator=g)

    def train_dataloader(self, shuffle=False):
        return self._loader(self.train_dataset, shuffle)

    def val_dataloader(self):
        return self._loader(self.val_dataset)

    def test_dataloader(self):
        return self._loader(self.test_dataset)
