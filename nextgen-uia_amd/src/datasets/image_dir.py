"""`--images DIR` of src/models/predict.py: a directory of pictures without lists, masks or labels, read the way src/datasets/folder.py reads the
reference's dataset folders.  A worker only DECODES (`Image.open(p).convert("L")`, the bytes at the file's own size); the collate packs a batch into the
ragged byte buffer and descriptor of uia_hip.ops.resize_batch with the square-squash geometry of the supervised loaders, so folder.RaggedPrefetcher and
folder.ResizeStage take it as it is.  The same device bytes are then the `src` of uia_hip.ops.seg_predict_native, which needs each image's own (H, W):
the collate hands them out beside the names.

The files of DIR itself (not of its sub-directories) with an image suffix, compared without case, sorted by name.  Sizes are read from the headers at
start-up; refused there, by name: a file the resize kernel's limits exclude (a downscale beyond 32x), a side above 16384 (the limit of
uia_seg_predict_native), two files with one stem (they would write the same output name).  Worker processes (at most 16) are started by start_workers(),
before the process initialises the GPU, and never after.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from src.datasets.folder import MAX_SIZE, MAX_WORKERS, MIN_SIZE, _pil, pack_ragged
from src.datasets.pil_resize import MAX_KSIZE, ksize_of

SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
MAX_SIDE = 16384


def list_images(folder):
    """The image files of `folder` itself, sorted by name."""
    return sorted(n for n in os.listdir(folder) if os.path.splitext(n)[1].lower() in SUFFIXES and os.path.isfile(os.path.join(folder, n)))


class ImageDir(Dataset):
    """sample = (gray bytes [H, W], name)."""

    def __init__(self, dir, img_size):
        Image = _pil()
        self.dir, self.img_size = str(dir), int(img_size)
        if not MIN_SIZE <= self.img_size <= MAX_SIZE:
            raise RuntimeError(f"--images: --img_size {img_size} is outside the resize kernel's limits ({MIN_SIZE} .. {MAX_SIZE})")
        self.names = list_images(self.dir)
        if not self.names:
            raise RuntimeError(f"--images: {self.dir} holds no image file ({' '.join(SUFFIXES)}; sub-directories are not read)")
        stems = {}
        for n in self.names:
            first = stems.setdefault(os.path.splitext(n)[0], n)
            if first != n:
                raise RuntimeError(f"--images: {first} and {n} share the stem {os.path.splitext(n)[0]!r} and would write the same output files")
        self.sizes = []                                         # (W, H) from the headers: nothing is decoded here
        for n in self.names:
            with Image.open(os.path.join(self.dir, n)) as im:
                W, H = im.size
            if max(W, H) > MAX_SIDE:
                raise RuntimeError(f"--images: {n} is {W} x {H}; the prediction kernel takes at most {MAX_SIDE} pixels a side")
            k = max(ksize_of(W, self.img_size), ksize_of(H, self.img_size))
            if k > MAX_KSIZE:
                raise RuntimeError(f"--images: {n} is {W} x {H}; resizing it to {self.img_size} x {self.img_size} takes {k} taps per pixel and the "
                                   f"resize kernel at most {MAX_KSIZE} (a downscale of at most 32x)")
            self.sizes.append((W, H))

    def __len__(self):
        return len(self.names)

    def name_of(self, i):
        return self.names[i]

    def __getitem__(self, i):
        Image = _pil()
        name = self.names[i]
        with Image.open(os.path.join(self.dir, name)) as im:
            return np.asarray(im.convert("L")), name


class ImageDirCollate:
    """samples -> (bytes uint8 [n], descriptor int32 [B, 8], None, (names, [(H, W)])): folder.RaggedCollate's tuple for a batch without masks or labels,
    with the images' own sizes beside their names."""

    def __init__(self, img_size):
        self.geom = (int(img_size), int(img_size), 0, 0)

    def __call__(self, samples):
        buf, desc = pack_ragged([(px, None, self.geom) for px, _ in samples])
        return buf, desc, None, ([name for _, name in samples], [tuple(px.shape[:2]) for px, _ in samples])


class ImageDirModule:
    """The loader of one prediction run: batches in file-name order, nothing dropped."""

    def __init__(self, dir, img_size, batch_size, num_workers=0):
        self.dataset = ImageDir(dir, img_size)
        self.batch_size = int(batch_size)
        nw = max(0, min(int(num_workers or 0), MAX_WORKERS))
        if nw and torch.cuda.is_initialized():                  # never fork after the GPU is up
            nw = 0
        kw = dict(num_workers=nw, drop_last=False, shuffle=False, collate_fn=ImageDirCollate(img_size))
        if nw:
            kw.update(persistent_workers=True, prefetch_factor=2)
        self.loader = DataLoader(self.dataset, batch_size=self.batch_size, **kw)

    def start_workers(self):
        if self.loader.num_workers > 0 and len(self.loader) > 0:
            self.loader._uia_first_iter = iter(self.loader)

    def shutdown(self):
        it = getattr(self.loader, "_iterator", None) or self.loader.__dict__.pop("_uia_first_iter", None)
        if it is not None and hasattr(it, "_shutdown_workers"):
            it._shutdown_workers()
        self.loader._iterator = None
