"""Training-time augmentation behind --strong_augs / --weak_augs (counterpart of the reference's src/datasets/segmentation.py:14-156,183-192 and
classification.py:14-151,183-192), split in two: the random DECISIONS are made here on the host, per batch, as a small program table; the PIXEL work
runs on the device in one launch per batch (uia_hip.ops.augment_batch, csrc/augment.hip) on the batch that the prefetcher has already copied.

The reference's decision structure, per training sample:
  * both flags on: a coin of 0.5 decides whether the sample is augmented at all; if so the strong augmentation runs, then the weak one.  One flag on: that
    augmentation always runs.
  * each augmentation draws n = randint(0, len(list) + 1) and picks n ops with replacement, applied in order.
  * strong (image only): identity, autocontrast, equalize, blur (sigma ~ U(0.75, 1.25)), contrast / brightness / sharpness (factor 1.25 - 0.5 u, u in
    [0, 1): (0.75, 1.25]), posterize to 8 - max(1, ceil(4 u)) bits, solarize at 256 - max(1, ceil(255 u)).
  * weak (image and mask): RandomResizedCrop(scale (0.8, 1.2), ratio 1) — torchvision's get_params: ten tries of side = round(sqrt(S^2 U(0.8, 1.2))),
    accepted when side <= S, with a uniform corner; the fallback is the whole image —, horizontal flip, vertical flip (always applied when chosen), identity.
So a program has at most 9 + 4 = 13 ops.  Validation and test batches are never augmented.

The draws come from a generator of their own, seeded from (--seed, rank, epoch, iteration): the global `random`, numpy and torch generators are never
touched, so model initialisation, shuffling and dropout draw what they drew before.  It is not the reference's stream (which interleaves `random`,
numpy and torch draws inside loader workers), only its distribution.

Program table: int32 [B, 14, 4]; row 0 of an image is (n, with_mask, 0, 0), rows 1 .. n are (opcode, p0, p1, p2), float parameters as float32 bit patterns.
"""
import math
import struct

import numpy as np

IDENTITY, AUTOCONTRAST, EQUALIZE, BLUR, CONTRAST, BRIGHTNESS, SHARPNESS, POSTERIZE, SOLARIZE, CROP, HFLIP, VFLIP = range(12)
STRONG_OPS = (IDENTITY, AUTOCONTRAST, EQUALIZE, BLUR, CONTRAST, BRIGHTNESS, SHARPNESS, POSTERIZE, SOLARIZE)      # reference get_strong_aug_list
WEAK_OPS = (CROP, HFLIP, VFLIP, IDENTITY)                                                                          # reference WeakAugmentation
MAX_OPS = len(STRONG_OPS) + len(WEAK_OPS)
ROWS = MAX_OPS + 1
CROP_TRIES = 10
_DRAWS = 2 + 2 * len(STRONG_OPS) + 1 + len(WEAK_OPS) * (1 + CROP_TRIES + 2)      # the most uniforms one sample can consume


def f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


def make_rng(seed, rank=0, epoch=0, iteration=0):
    """The stage's own generator for one batch."""
    return np.random.default_rng([int(seed), int(rank), int(epoch), int(iteration)])


def crop_params(S, nxt, scale=(0.8, 1.2)):
    """torchvision RandomResizedCrop.get_params at ratio (1, 1) on an S x S image -> (i, j, side).  nxt() yields U[0, 1)."""
    for _ in range(CROP_TRIES):
        side = int(round(math.sqrt(S * S * (scale[0] + (scale[1] - scale[0]) * nxt()))))
        if 0 < side <= S:
            return int(nxt() * (S - side + 1)), int(nxt() * (S - side + 1)), side
    return 0, 0, S                                              # the fallback: the whole image (ratio 1 lies inside [1, 1])


def _strong_op(code, nxt):
    if code == BLUR:
        return (code, f32_bits(0.75 + 0.5 * nxt()), 0, 0)
    if code in (CONTRAST, BRIGHTNESS, SHARPNESS):
        return (code, f32_bits(1.25 - 0.5 * nxt()), 0, 0)
    if code == POSTERIZE:
        return (code, 8 - max(1, int(math.ceil(4 * nxt()))), 0, 0)
    if code == SOLARIZE:
        return (code, 256 - max(1, int(math.ceil(255 * nxt()))), 0, 0)
    return (code, 0, 0, 0)


def draw_program(S, strong, weak, nxt, crop_scale=(0.8, 1.2)):
    """The op rows of one training sample."""
    rows = []
    if not (strong or weak) or (strong and weak and not nxt() < 0.5):
        return rows
    if strong:
        for _ in range(int(nxt() * (len(STRONG_OPS) + 1))):
            rows.append(_strong_op(STRONG_OPS[int(nxt() * len(STRONG_OPS))], nxt))
    if weak:
        for _ in range(int(nxt() * (len(WEAK_OPS) + 1))):
            code = WEAK_OPS[int(nxt() * len(WEAK_OPS))]
            rows.append((code,) + (crop_params(S, nxt, crop_scale) if code == CROP else (0, 0, 0)))
    return rows


def draw_programs(B, S, strong, weak, with_mask, rng, out=None, crop_scale=(0.8, 1.2)):
    """The program table of a batch of B training samples of S x S pixels, int32 [B, 14, 4] (written into `out` when given: the pinned table that travels
    to the device).  One bulk draw of uniforms from `rng`; sample b consumes row b only, so its program does not depend on its neighbours."""
    table = np.zeros((B, ROWS, 4), dtype=np.int32) if out is None else out
    assert table.shape == (B, ROWS, 4) and table.dtype == np.int32
    table[...] = 0
    u = rng.random((B, _DRAWS)).tolist()
    for b in range(B):
        rows = draw_program(S, strong, weak, iter(u[b]).__next__, crop_scale)
        table[b, 0, 0], table[b, 0, 1] = len(rows), int(bool(with_mask))
        if rows:
            table[b, 1:1 + len(rows)] = rows
    return table


class BatchAugmenter:
    """The stage of a training loop: `images, masks = stage(images, masks)` right behind the prefetcher's event, before the batch reaches the model.
    One table draw on the host, one asynchronous table copy and one kernel launch on the current stream; the outputs, the scratch and a small ring of
    pinned tables are allocated once.  `augmented` counts the training images with a non-empty program."""

    DEPTH = 8                                                   # pinned tables in flight: the host never runs this many batches ahead of the device

    def __init__(self, strong, weak, with_mask, seed, rank=0):
        self.strong, self.weak, self.with_mask, self.seed, self.rank = bool(strong), bool(weak), bool(with_mask), int(seed), int(rank)
        self.epoch, self.iteration, self.augmented = 0, 0, 0
        self._shape, self._tables, self._events, self._k = None, None, None, 0
        self._out_i = self._out_m = self._ws = None

    def set_epoch(self, epoch):
        self.epoch, self.iteration = int(epoch), 0

    def _alloc(self, images, masks):
        import torch
        from uia_hip import ops
        B, _, S, _ = images.shape
        if self._tables is not None:
            torch.cuda.current_stream().synchronize()          # a batch shape changed mid-run: no table copy may be in flight when its memory goes
        self._shape = tuple(images.shape)
        self._tables = [torch.zeros(B, ROWS, 4, dtype=torch.int32, pin_memory=True) for _ in range(self.DEPTH)]
        self._events = [None] * self.DEPTH
        self._out_i = torch.empty_like(images)
        self._out_m = None if masks is None else torch.empty_like(masks)
        self._ws = ops.augment_workspace(B, S, images.device)

    def __call__(self, images, masks=None):
        import torch
        from uia_hip import ops
        if images.dim() != 4 or images.shape[1] != 1 or images.dtype != torch.float32:
            raise ValueError(f"augmentation takes the one-channel fp32 batch of the dataset modules, got {images.dtype} {tuple(images.shape)}")
        if images.shape[2] != images.shape[3] or not 8 <= images.shape[2] <= 1024:
            raise ValueError(f"--strong_augs / --weak_augs take square images of 8 to 1024 pixels a side, got {tuple(images.shape[2:])} "
                             "(resize the --data_pt file, or pass --no-strong_augs --no-weak_augs)")
        if self.with_mask != (masks is not None):
            raise ValueError("the stage was made for batches " + ("with" if self.with_mask else "without") + " masks")
        if self._shape != tuple(images.shape) or (masks is None) != (self._out_m is None):
            self._alloc(images, masks)
        k = self._k % self.DEPTH
        self._k += 1
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        else:
            self._events[k].synchronize()                      # the copy of DEPTH batches ago: long done
        B, _, S, _ = images.shape
        table = self._tables[k]
        draw_programs(B, S, self.strong, self.weak, self.with_mask, make_rng(self.seed, self.rank, self.epoch, self.iteration), out=table.numpy())
        self.iteration += 1
        self.augmented += int(np.count_nonzero(table.numpy()[:, 0, 0]))
        ops.augment_batch(images, masks, table, self._out_i, self._out_m, self._ws)
        self._events[k].record()
        return self._out_i, self._out_m


def stage_for(args, with_mask, rank=0):
    """The training loops' switch: a BatchAugmenter when a flag is on and the data comes from --data_pt (the DataModules take it before --synthetic) or
    from --data_root (taken after both),
    else None — runs on the `--synthetic` noise (timing and tests) and `--no-strong_augs --no-weak_augs` bypass the stage entirely: no launch, the same
    bits as without it.  The stage takes square images of 8 to 1024 pixels a side in [0, 1] (BatchAugmenter refuses other shapes at the first batch)."""
    strong, weak = bool(getattr(args, "strong_augs", False)), bool(getattr(args, "weak_augs", False))
    folders = getattr(args, "data_root", None) and not getattr(args, "synthetic", False)      # src/datasets/folder.py: its ResizeStage yields a --data_pt batch
    if not (strong or weak) or not (getattr(args, "data_pt", None) or folders):
        return None
    return BatchAugmenter(strong, weak, with_mask, getattr(args, "seed", 0), rank)
