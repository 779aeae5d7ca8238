"""The device-resident training set of the few-shot entries.  A few-shot training list is a handful of images (1 % of a list; K per class), sampled
once: it is uploaded once, as stored (uint8 files stay uint8), and every training batch is formed on the device by ONE launch — uia_augment_gather
(csrc/augment.hip) gathers the epoch's permuted rows, runs each row's augmentation program and writes the fp32 batch and its masks.  No loader
workers, no shared-memory ring, no per-batch host-to-device copy of pixels, no separate gather pass.

`ResidentTrainSet` hands the loop `(images, labels, ready)` as engine.DevicePrefetcher does.  The batch contract is the reference's few-shot loader
(src/datasets/fewshot_*.py train_dataloader): B = min(batch_size, n), drop_last = n > batch_size, a fresh permutation per epoch — so every batch has
exactly B rows and an epoch has n // B of them.  The permutation comes from a generator seeded by (seed, epoch): the reference's distribution, not
its stream (torch's global generator inside the DataLoader), as with the augmentation draws.  The programs are drawn as src/datasets/augment.py
draws them, from the same (seed, rank, epoch, iteration) generator; the `src` column of row 0 is then written into the pinned table.  With the stage
off (`--synthetic`, or `--no-strong_augs --no-weak_augs`) every program is empty and the launch is a pure gather: there is no second code path.
Class labels are gathered with torch.index_select; masks travel through the kernel.
"""
import numpy as np

from src.datasets.augment import ROWS, draw_programs, make_rng


def batch_plan(n, batch_size):
    """(B, iterations per epoch) of the reference's few-shot training loader over n samples."""
    if n < 1 or batch_size < 1:
        raise ValueError(f"a resident training set needs at least one row and a batch size of at least 1 (n={n}, batch_size={batch_size})")
    B = min(batch_size, n)
    return B, n // B


def epoch_permutation(n, seed, epoch):
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n)


class ResidentTrainSet:
    DEPTH = 8                                                   # pinned tables in flight, as BatchAugmenter

    def __init__(self, images, second, batch_size, strong=False, weak=False, seed=0, rank=0, device="cuda", launch=None):
        """images [n, 1, S, S] uint8 or fp32, second: masks uint8 [n, 1, S, S] (they follow the geometry ops) or class labels int64 [n].
        launch(images, masks, table, out_images, out_masks, ws): uia_hip.ops.augment_gather unless given (the host tests count calls with a stub)."""
        import torch
        if images.dim() != 4 or images.shape[1] != 1 or images.shape[2] != images.shape[3] or not 8 <= images.shape[2] <= 1024:
            raise ValueError(f"the resident training set takes square one-channel images of 8 to 1024 pixels a side, got {tuple(images.shape)}")
        if images.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"the resident training set takes uint8 or fp32 images, got {images.dtype}")
        self.n, self.S = int(images.shape[0]), int(images.shape[2])
        self.B, self.iters = batch_plan(self.n, int(batch_size))
        self.with_mask = second.dim() == 4
        if (self.with_mask and (second.shape != images.shape or second.dtype != torch.uint8)) or (not self.with_mask and tuple(second.shape) != (self.n,)):
            raise ValueError(f"masks must be uint8 {tuple(images.shape)}, class labels [{self.n}]; got {second.dtype} {tuple(second.shape)}")
        self.strong, self.weak, self.seed, self.rank = bool(strong), bool(weak), int(seed), int(rank)
        self.device = torch.device(device)
        self.on_gpu = self.device.type == "cuda"
        self.images = images.contiguous().to(self.device)      # the one upload
        self.second = second.contiguous().to(self.device)
        self.epoch, self.augmented, self.wait_s = 0, 0, 0.0
        self._tables = [torch.zeros(self.B, ROWS, 4, dtype=torch.int32, pin_memory=self.on_gpu) for _ in range(self.DEPTH)]
        self._events, self._k = [None] * self.DEPTH, 0
        self._perm_host = torch.zeros(self.n, dtype=torch.int64, pin_memory=self.on_gpu)
        self._out_i = torch.empty(self.B, 1, self.S, self.S, dtype=torch.float32, device=self.device)
        self._out_m = torch.empty(self.B, 1, self.S, self.S, dtype=torch.uint8, device=self.device) if self.with_mask else None
        self._ws = None
        if launch is None:
            from uia_hip import ops
            launch = ops.augment_gather
            self._ws = ops.augment_workspace(self.B, self.S, self.device)
        self._launch = launch

    def __len__(self):
        return self.iters

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def close(self):
        pass

    def __iter__(self):
        import torch
        perm = epoch_permutation(self.n, self.seed, self.epoch)
        perm_dev = None
        if not self.with_mask:
            if self.on_gpu:
                torch.cuda.current_stream().synchronize()     # the previous epoch's copy of the pinned permutation has run before it is rewritten
            self._perm_host.copy_(torch.from_numpy(perm))
            perm_dev = self._perm_host.to(self.device, non_blocking=True)
        for it in range(self.iters):
            k = self._k % self.DEPTH
            self._k += 1
            if self.on_gpu:
                if self._events[k] is None:
                    self._events[k] = torch.cuda.Event()
                else:
                    self._events[k].synchronize()              # the table copy of DEPTH batches ago: long done
            table = self._tables[k]
            t = table.numpy()
            draw_programs(self.B, self.S, self.strong, self.weak, self.with_mask, make_rng(self.seed, self.rank, self.epoch, it), out=t)
            t[:, 0, 2] = perm[it * self.B:(it + 1) * self.B]
            self.augmented += int(np.count_nonzero(t[:, 0, 0]))
            self._launch(self.images, self.second if self.with_mask else None, table, self._out_i, self._out_m, self._ws)
            labels = self._out_m if self.with_mask else torch.index_select(self.second, 0, perm_dev[it * self.B:(it + 1) * self.B])
            if self.on_gpu:
                self._events[k].record()
            yield self._out_i, labels, self._events[k]


def resident_for(args, dm, rank=0):
    """The few-shot loops' training source: the data module's sampled rows on args.device; the stage is on under the conditions of augment.stage_for."""
    strong, weak = bool(getattr(args, "strong_augs", False)), bool(getattr(args, "weak_augs", False))
    on = bool(getattr(args, "data_pt", None))
    images, second = dm.resident_rows()
    return ResidentTrainSet(images, second, args.batch_size, strong and on, weak and on, getattr(args, "seed", 0), rank, args.device)
