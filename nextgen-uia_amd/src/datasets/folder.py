"""`--data_root DIR`: the reference's dataset folders read as they are released (reference src/datasets/segmentation.py:159-251, classification.py:157-251,
which hard-wire ../data/NextGen-UIA):

    DIR/{classification,segmentation}/<dataset>/{train,val,test}.txt     one file name per line
    DIR/classification/<dataset>/labels.csv                              csv.reader rows: row[0] -> int(row[1])
    DIR/all/images/<name>, DIR/all/masks/<name>

The reference's worker does, per sample, Image.open(p).convert("L") (masks: .convert("1")), .resize((S, S)), the augmentations, ToTensor and the repeat
to three channels.  Here a worker only DECODES: `__getitem__` makes the two PIL calls and returns the bytes at the file's own size.  The collate packs
a batch into one ragged byte buffer plus a descriptor (uia_hip.ops.resize_batch's), `RaggedPrefetcher` copies it to the device, and `ResizeStage` —
right behind the prefetcher's event, before the augmentation stage — turns it into the batch a `--data_pt` file of the same pictures gives, bit for
bit: one launch of uia_resize_batch (csrc/resize.hip), which is PIL's resize in every byte (src/datasets/pil_resize.py restates it).

Image sizes are read from the file headers at start-up; a file the kernel's limits exclude (a downscale beyond 32x, a mask whose size is not its
image's) is refused there, by name.  PIL is imported when the first folder is opened.  Worker processes (at most 16) are started by start_workers(),
before the process initialises the GPU, and never after: a module made later loads in-process.
"""
import csv
import os
import threading
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from src.datasets.finetune import RankShardSampler
from src.datasets.pil_resize import MAX_KSIZE, ksize_of

DESC = 8                                                        # int32 per image: offset, H, W, mask offset or -1, dst_h, dst_w, y0, x0
MAX_WORKERS = 16
MIN_SIZE, MAX_SIZE = 8, 1024                                    # img_size the kernel takes
OUT_OF_SCOPE = ("--data_root reads the reference's dataset folders for the supervised classification and segmentation entries only; {what} takes "
                "--synthetic or --data_pt (DESIGN.md, \"Not built\"){hint}")
CAPTION_HINT = "; the caption folders of the contrastive fine-tune are read with --finetune_root"


def _pil():
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("--data_root decodes the dataset's image files with Pillow, which is not installed (pip install pillow); "
                           "--data_pt takes a pre-converted tensor file instead") from e
    return Image


def chosen(args):
    """The DataModules' precedence: --data_pt, then --synthetic, then --data_root."""
    return bool(getattr(args, "data_root", None)) and not getattr(args, "data_pt", None) and not getattr(args, "synthetic", False)


def refuse(args, what):
    """Entry points outside this loader's scope call this before anything else."""
    if getattr(args, "data_root", None):
        raise RuntimeError(OUT_OF_SCOPE.format(what=what, hint=CAPTION_HINT if "contrastive" in what else ""))


def pack_ragged(items):
    """items: [(pixels uint8 [H, W] or [H, W, C], mask uint8 / bool [H, W] or None, (dst_h, dst_w, y0, x0))] -> (one uint8 tensor holding every image
    and mask back to back, the int32 descriptor [B, 8] of uia_hip.ops.resize_batch)."""
    desc = torch.zeros(len(items), DESC, dtype=torch.int32)
    total = sum(px.size + (0 if m is None else m.size) for px, m, _ in items)
    buf = torch.empty(total, dtype=torch.uint8)
    flat, at = buf.numpy(), 0
    for b, (px, mask, geom) in enumerate(items):
        H, W = px.shape[:2]
        flat[at:at + px.size] = px.reshape(-1)
        off, at, moff = at, at + px.size, -1
        if mask is not None:
            if mask.shape != (H, W):
                raise ValueError(f"sample {b}: a {mask.shape} mask beside a {(H, W)} image")
            flat[at:at + mask.size] = mask.reshape(-1)
            moff, at = at, at + mask.size
        desc[b] = torch.tensor([off, H, W, moff, *geom], dtype=torch.int32)
    return buf, desc


class FolderSplit(Dataset):
    """One split of one dataset.  kind "segmentation": sample = (gray bytes [H, W], mask bytes [H, W], zero or not, name); "classification": (gray bytes,
    int label, name)."""

    def __init__(self, root, kind, dataset, split, img_size):
        Image = _pil()
        self.root, self.kind, self.img_size = root, kind, int(img_size)
        if not MIN_SIZE <= self.img_size <= MAX_SIZE:
            raise RuntimeError(f"--data_root: --img_size {img_size} is outside the resize kernel's limits ({MIN_SIZE} .. {MAX_SIZE})")
        folder = os.path.join(root, kind, dataset)
        with open(os.path.join(folder, f"{split}.txt")) as f:
            self.names = f.read().splitlines()
        self.labels = None
        if kind == "classification":
            with open(os.path.join(folder, "labels.csv")) as f:
                table = {str(row[0]): int(row[1]) for row in csv.reader(f)}
            self.labels = [table[n] for n in self.names]
        self.sizes = []                                         # (W, H) from the headers: nothing is decoded here
        for n in self.names:
            with Image.open(self.image_path(n)) as im:
                W, H = im.size
            if kind == "segmentation":
                with Image.open(self.mask_path(n)) as m:
                    if m.size != (W, H):
                        raise RuntimeError(f"--data_root: the mask of {n} is {m.size[0]} x {m.size[1]}, its image {W} x {H}: one descriptor carries both")
            k = max(ksize_of(W, self.img_size), ksize_of(H, self.img_size))
            if k > MAX_KSIZE:
                raise RuntimeError(f"--data_root: {n} is {W} x {H}; resizing it to {self.img_size} x {self.img_size} takes {k} taps per pixel and the "
                                   f"resize kernel at most {MAX_KSIZE} (a downscale of at most 32x)")
            self.sizes.append((W, H))

    def image_path(self, name):
        return os.path.join(self.root, "all", "images", name)

    def mask_path(self, name):
        return os.path.join(self.root, "all", "masks", name)

    def __len__(self):
        return len(self.names)

    def name_of(self, i):
        return self.names[i]

    def __getitem__(self, i):
        Image = _pil()
        name = self.names[i]
        with Image.open(self.image_path(name)) as im:
            px = np.asarray(im.convert("L"))
        if self.kind == "classification":
            return px, self.labels[i], name
        with Image.open(self.mask_path(name)) as m:
            mask = np.asarray(m.convert("1")).view(np.uint8)    # Pillow hands a mode "1" image out as bool, one byte per pixel (0 or 255)
        return px, mask, name


class RaggedCollate:
    """samples -> (bytes uint8 [n], descriptor int32 [B, 8], labels int64 [B] or None, names): the square squash of the supervised loaders."""

    def __init__(self, img_size, kind):
        self.geom, self.kind = (int(img_size), int(img_size), 0, 0), kind

    def __call__(self, samples):
        seg = self.kind == "segmentation"
        buf, desc = pack_ragged([(s[0], s[1] if seg else None, self.geom) for s in samples])
        labels = None if seg else torch.tensor([s[1] for s in samples], dtype=torch.int64)
        return buf, desc, labels, [s[2] for s in samples]


class DataModule:
    """The interface src/models/supervised.py drives (src/datasets/segmentation.DataModule's), over FolderSplit."""

    def __init__(self, args, kind, rank=0, world=1):
        self.args, self.kind, self.rank, self.world = args, kind, rank, world
        mk = lambda split: FolderSplit(args.data_root, kind, args.dataset, split, args.img_size)
        self.train_dataset, self.val_dataset, self.test_dataset = mk("train"), mk("val"), mk("test")
        self.train_sampler = None
        self._loaders = []

    def _loader(self, ds, train):
        a = self.args
        nw = max(0, min(int(getattr(a, "num_workers", 0) or 0), MAX_WORKERS if train else 2))
        if nw and torch.cuda.is_initialized():                  # never fork after the GPU is up
            nw = 0
        kw = dict(num_workers=nw, drop_last=train, collate_fn=RaggedCollate(a.img_size, self.kind))
        if nw:
            kw.update(persistent_workers=True, prefetch_factor=2)
        if train and self.world > 1:
            self.train_sampler = RankShardSampler(len(ds), self.rank, self.world, shuffle=True, seed=getattr(a, "seed", 0), drop_last=True)
            loader = DataLoader(ds, batch_size=a.batch_size, sampler=self.train_sampler, **kw)
        else:
            loader = DataLoader(ds, batch_size=a.batch_size, shuffle=train, **kw)
        self._loaders.append(loader)
        return loader

    def train_dataloader(self):
        return self._loader(self.train_dataset, True)

    def val_dataloader(self):
        return self._loader(self.val_dataset, False)

    def test_dataloader(self):
        return self._loader(self.test_dataset, False)

    def start_workers(self):
        for loader in self._loaders:
            if loader.num_workers > 0 and len(loader) > 0:
                loader._uia_first_iter = iter(loader)

    def set_epoch(self, epoch):
        if self.train_sampler is not None:
            self.train_sampler.set_epoch(epoch)

    def shutdown(self):
        for loader in self._loaders:
            it = getattr(loader, "_iterator", None) or loader.__dict__.pop("_uia_first_iter", None)
            if it is not None and hasattr(it, "_shutdown_workers"):
                it._shutdown_workers()
            loader._iterator = None


class RaggedBatch:
    """What RaggedPrefetcher yields in the images' place: the device bytes and the (pinned) host descriptor of one batch."""

    def __init__(self, data, desc):
        self.data, self.desc = data, desc


class RaggedPrefetcher:
    """engine.DevicePrefetcher's interface — `for batch, second, ready in pf`, `wait_s`, `len`, `close()` — for RaggedCollate batches: a background
    thread stages a batch's bytes and descriptor in pinned memory and copies the bytes (and the labels) to the device on a copy stream; `batch` is a
    RaggedBatch for ResizeStage, `second` the int64 labels on the device (classification) or None (segmentation: the masks are in the bytes).  A slot's
    pinned and device memory is reused only behind the event the consumer's stream records when it asks for the next batch."""

    def __init__(self, loader, device, depth=2):
        self.loader, self.device, self.depth = loader, torch.device(device), max(1, depth)
        self.wait_s = 0.0
        self._slots = [None] * (self.depth + 2)
        self._copy = torch.cuda.Stream(device=self.device)
        self._stop = threading.Event()
        self._live = None

    def __len__(self):
        return len(self.loader)

    def _slot(self, k, nbytes, B):
        s = self._slots[k]
        if s is not None and s["free"] is not None:
            s["free"].synchronize()                             # the consumer's last reader of this slot (its descriptor copy included)
        if s is None or s["h"].numel() < nbytes or s["h_desc"].shape[0] < B:
            cap = max(nbytes + nbytes // 4, 1 << 16)
            s = {"h": torch.empty(cap, dtype=torch.uint8, pin_memory=True), "d": torch.empty(cap, dtype=torch.uint8, device=self.device),
                 "h_desc": torch.empty(B, DESC, dtype=torch.int32, pin_memory=True), "h_lab": torch.empty(B, dtype=torch.int64, pin_memory=True),
                 "d_lab": torch.empty(B, dtype=torch.int64, device=self.device), "free": None}
            self._slots[k] = s
        return s

    def _producer(self, it, q):
        try:
            torch.cuda.set_device(self.device)
            k = 0
            for buf, desc, labels, _names in it:
                n, B = buf.numel(), desc.shape[0]
                s = self._slot(k % len(self._slots), n, B)
                k += 1
                s["h"][:n].copy_(buf)
                s["h_desc"][:B].copy_(desc)
                second = None
                with torch.cuda.stream(self._copy):
                    s["d"][:n].copy_(s["h"][:n], non_blocking=True)
                    if labels is not None:
                        s["h_lab"][:B].copy_(labels)
                        s["d_lab"][:B].copy_(s["h_lab"][:B], non_blocking=True)
                        second = s["d_lab"][:B]
                    ev = torch.cuda.Event()
                    ev.record(self._copy)
                ev.synchronize()                                # the pinned bytes may be rewritten once this slot comes round again
                if not self._put(q, (s, RaggedBatch(s["d"][:n], s["h_desc"][:B]), second, ev)):
                    break
            self._put(q, None)
        except BaseException as e:                              # surfaces in the consumer
            self._put(q, e)

    def _put(self, q, item):
        import queue
        while not self._stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def close(self):
        live, self._live = self._live, None
        if live is None:
            return
        th, q = live
        self._stop.set()
        while th.is_alive():
            try:
                q.get(timeout=0.05)
            except Exception:
                pass
            th.join(timeout=0.05)
        self._stop.clear()

    def __iter__(self):
        import queue
        q = queue.Queue(maxsize=self.depth)
        first = self.loader.__dict__.pop("_uia_first_iter", None)
        self.close()
        th = threading.Thread(target=self._producer, args=(first if first is not None else iter(self.loader), q), daemon=True)
        th.start()
        self._live = (th, q)
        return self._consume(th, q)

    def _consume(self, th, q):
        prev = None
        while True:
            if prev is not None:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                prev["free"] = ev
                prev = None
            t0 = time.perf_counter()
            item = q.get()
            self.wait_s += time.perf_counter() - t0
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            prev, batch, second, ev = item
            yield batch, second, ev
        th.join()
        if self._live is not None and self._live[0] is th:
            self._live = None


class ResizeStage:
    """`images, second = stage(batch, second)` behind the prefetcher's event: one uia_resize_batch launch on the current stream -> images fp32
    [B, 1, S, S] in [0, 1] and, for segmentation, the masks uint8 [B, 1, S, S] in {0, 1} (classification: `second`, the labels, passes through) —
    the batch of a --data_pt file holding the same pictures resized by PIL.  Outputs and workspace are allocated once per batch size."""

    def __init__(self, img_size, with_mask):
        self.S, self.with_mask = int(img_size), bool(with_mask)
        self._bufs = {}

    def __call__(self, batch, second=None):
        from uia_hip import ops
        B = batch.desc.shape[0]
        if B not in self._bufs:
            dev = batch.data.device
            self._bufs[B] = (torch.empty(B, 1, self.S, self.S, dtype=torch.float32, device=dev),
                             torch.empty(B, 1, self.S, self.S, dtype=torch.uint8, device=dev) if self.with_mask else None, ops.resize_workspace(B, dev))
        out_i, out_m, ws = self._bufs[B]
        ops.resize_batch(batch.data, batch.desc, self.S, 1, out_i, out_m, ws)
        return out_i, (out_m if self.with_mask else second)


def stage_for(args, with_mask):
    """The loops' switch: a ResizeStage when the data comes from --data_root, else None."""
    return ResizeStage(args.img_size, with_mask) if chosen(args) else None
