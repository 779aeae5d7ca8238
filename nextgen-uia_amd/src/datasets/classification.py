"""Image / label data for the classification entry points (counterpart of the reference's src/datasets/classification.py).

The reference reads grayscale PNGs listed in ../data/NextGen-UIA/classification/<dataset>/{train,val,test}.txt with labels from labels.csv, augments them
with PIL / torchvision (:14-147) and hands batches of (image float32 [B, 3, S, S] in [0, 1] — ONE grayscale channel repeated, :183, :201-203 — label int64 [B],
file names) to the loop, `shuffle=True, drop_last=True` for training and neither for validation / test (:232-262).  `--data_root DIR` reads those folders as
they are (src/datasets/folder.py: the workers decode, PIL's resize runs on the device, one launch per batch, equal to PIL in every byte) and yields the batch
a `--data_pt` file of the same pictures yields; this module serves `--synthetic` and `--data_pt`: that batch contract and the three splits.  The augmentation (:14-151,
`--strong_augs` / `--weak_augs`) is not done here: `__getitem__` returns the plain sample, and the training loop runs it on the device on the copied batch
(src/datasets/augment.py: decisions on the host, pixels in one launch per batch; `--data_pt` and `--data_root` batches only).  With a flag on (the default) a `--data_pt` file must hold SQUARE images of 8 to 1024 pixels a side
(anything else is refused at the first training batch: resize the file or pass `--no-strong_augs --no-weak_augs`), and float images are taken to lie in
[0, 1]: an augmented sample is quantised to 8 bits, which clamps values outside it, while an untouched sample of the same batch passes as it is.

`--synthetic` supplies them deterministically by seed and balanced (even indices class 0, odd indices class 1): every image is U[0,1) texture scaled by 0.6;
a class-1 image also carries a bright axis-aligned ellipse (the synthetic lesion of src/datasets/segmentation.py), so the classes are learnable.
`--data_pt` takes real data as a .pt file of {"images": uint8 [N, 1 or 3, S, S], "labels": [N], optional "names", optional "split": {"train": idx,
"val": idx, "test": idx}} — without "split", 70 / 10 / 20 in file order.

A split lives in memory as tensors and a batch is an index gather, so loading runs in this process; a batch travels host -> device as ONE channel
(float32, the towers' patch embedding takes it with the channel-summed kernel, uia_hip.functional.gray_conv_weight) plus its int64 labels through
engine.DevicePrefetcher (`second=second_of`)."""
import torch
from torch.utils.data import DataLoader, Dataset


def synthetic_split(n, size, seed):
    """(images float32 [n, 1, S, S] in [0, 1], labels int64 [n]): labels alternate 0, 1; class 1 carries an ellipse of brightness 0.9 + texture·0.1."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(n, 1, size, size, generator=g) * 0.6
    labels = torch.arange(n, dtype=torch.int64) % 2
    c = torch.rand(n, 2, generator=g) * size * 0.5 + size * 0.25
    r = torch.rand(n, 2, generator=g) * size * 0.15 + size * 0.12
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    inside = (((yy[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((xx[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2) <= 1
    lesion = inside & (labels[:, None, None] == 1)
    img[:, 0] = torch.where(lesion, 0.9 + img[:, 0] / 6, img[:, 0])
    return img, labels


class TensorClassification(Dataset):
    def __init__(self, images, labels, names):
        self.images, self.labels, self.names = images, labels, names

    def __len__(self):
        return len(self.names)

    def name_of(self, i):
        return self.names[i]

    def __getitem__(self, i):
        img = self.images[i]
        img = img.float() / 255.0 if img.dtype == torch.uint8 else img.float()
        return img[:1], self.labels[i], self.names[i]          # the reference converts every image to one grayscale channel (:180)


def _collate(samples):
    return torch.stack([s[0] for s in samples]), torch.stack([s[1] for s in samples]).to(torch.int64), [s[2] for s in samples]


def second_of(batch):
    """What engine.DevicePrefetcher copies beside the images: the labels."""
    return batch[1]


class DataModule:
    def __init__(self, args, rank=0, world=1):
        """rank / world and start_workers() / shutdown() are the segmentation DataModule's interface (src/models/supervised.py drives both): a split is
        loaded in this process whole, so there is no shard and nothing to fork or stop."""
        self.args = args
        if getattr(args, "data_pt", None):
            blob = torch.load(args.data_pt)
            n = len(blob["images"])
            names = list(blob.get("names") or [f"{i:05d}.png" for i in range(n)])
            labels = torch.as_tensor(blob["labels"]).reshape(n).to(torch.int64)
            split = blob.get("split")
            if split is None:                                   # 70 / 10 / 20 in file order (the reference's lists are pre-shuffled text files)
                a, b = int(n * 0.7), int(n * 0.8)
                split = {"train": list(range(a)), "val": list(range(a, b)), "test": list(range(b, n))}
            mk = lambda idx: TensorClassification(blob["images"][list(idx)], labels[list(idx)], [names[i] for i in idx])
            self.train_dataset, self.val_dataset, self.test_dataset = mk(split["train"]), mk(split["val"]), mk(split["test"])
        elif getattr(args, "synthetic", False):
            mk = lambda n, seed, prefix: TensorClassification(*synthetic_split(n, args.img_size, seed), [f"{prefix}_{i:05d}.png" for i in range(n)])
            self.train_dataset = mk(args.synthetic_train, args.seed, "train")
            self.val_dataset = mk(args.synthetic_val, args.seed + 1, "val")
            self.test_dataset = mk(args.synthetic_test, args.seed + 2, "test")
        else:
            raise RuntimeError("no dataset: pass --synthetic, --data_pt or --data_root (the reference's folders, ../data/NextGen-UIA there, are read by src/datasets/folder.py)")

    def _loader(self, ds, train):
        return DataLoader(ds, batch_size=self.args.batch_size, shuffle=train, drop_last=train, num_workers=0, collate_fn=_collate)

    def train_dataloader(self):
        return self._loader(self.train_dataset, True)

    def val_dataloader(self):
        return self._loader(self.val_dataset, False)

    def test_dataloader(self):
        return self._loader(self.test_dataset, False)

    def start_workers(self):
        pass

    def shutdown(self):
        pass
