"""`--finetune_root DIR`: the reference's caption folders read as they are released (reference src/datasets/finetune.py:69-122, which hard-wires
/root/project/data/NextGen-UIA/finetune):

    DIR/medpix_dataset/medpix_dataset.csv       DIR/medpix_dataset/images/<file>
    DIR/pmc_curd_dataset/pmc_curd_dataset.csv   DIR/pmc_curd_dataset/images/<file>          columns: Caption, filename

Either dataset may be absent.  The preparation is the reference's: captions cleaned with its pattern, stripped, kept when longer than 20 characters;
a row's file is basename(filename) looked up in the two image folders in that order, rows without one dropped with the reference's warning; the
rows shuffled with numpy.random.RandomState(seed).permutation(n) — what pandas' df.sample(frac=1, random_state=seed) draws — and cut 90 / 10.

The reference's worker does Image.open -> convert("RGB") when the mode is not RGB -> Resize(S, BICUBIC) -> CenterCrop(S) -> ToTensor per sample.
Here a worker only DECODES: mode "L" files as one channel, "RGB" files as three, every other mode through convert("RGB"), at the file's own size.
`geometry` is the shorter-side rule and the crop window; the pixels are made on the device by one uia_resize_batch_rgb launch per batch
(csrc/resize.hip), which equals Pillow in every byte.  An image the kernel cannot take — a downscale beyond 32x on the short side, or more than
IMAGE_LIMIT decoded bytes — is resized by Pillow in the worker and shipped at its resized size (cropped to the window if that is still above the
limit), with a descriptor whose resize is the identity: the batch is the same either way.

Batches travel through `ByteSlotRing`: slots of batch x IMAGE_LIMIT bytes in shared memory, allocated once before the workers are forked; a
worker's collate writes bytes, descriptor and token ids straight into a free slot.  `CaptionPrefetcher` (engine.DevicePrefetcher's interface)
registers the ring as pinned memory once the GPU is up, copies from the slot on a copy stream and hands a slot back only behind the consumer's
event; `RgbResizeStage` turns the ragged batch into the [B, 3, S, S] batch the loop takes.  An abandoned iteration returns its slots: the batch
sampler is stopped and the batches already in flight are drained (`ByteSlotRing.drain`).
"""
import csv
import logging
import os
import queue
import re
import threading
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from src.datasets.finetune import RankShardSampler
from src.datasets.folder import DESC, MAX_SIZE, MIN_SIZE, _pil
from src.datasets.pil_resize import MAX_KSIZE, ksize_of

DATASETS = ("medpix_dataset", "pmc_curd_dataset")
CAPTION_KEY, IMAGE_KEY = "Caption", "filename"
MIN_CAPTION = 20                                                # captions must be LONGER than this
# the characters the reference keeps (datasets/finetune.py:91-93): letters, digits, white space, common punctuation and a few scientific symbols
CLEAN = re.compile("[^A-Za-z0-9\\s.,;:()\\[\\]{}/_\\-+*=<>@&|\\\\^'\"`~$?#!…±°µμ≤≥≈→–—•]")
IMAGE_LIMIT = 1 << 20                                           # decoded bytes of one image in a slot: 1024 x 1024 gray, 682 x 512 RGB
MAX_WORKERS = 16
MAX_DST = 16384                                                 # pixels a side the kernel resamples to, at most


def chosen(args):
    """The precedence: --data_pt, then --synthetic, then --finetune_root."""
    return bool(getattr(args, "finetune_root", None)) and not getattr(args, "data_pt", None) and not getattr(args, "synthetic", False)


def image_limit(img_size):
    """Bytes a slot reserves per image: IMAGE_LIMIT, and never less than the S x S x 3 window an oversized image is cut down to at worst."""
    return max(IMAGE_LIMIT, 3 * int(img_size) ** 2)


def geometry(W, H, S):
    """(dst_h, dst_w, y0, x0) of torchvision's Resize(S) + CenterCrop(S) on a W x H image.  Resize (torchvision/transforms/functional.py,
    _compute_resized_output_size): the shorter side becomes S, the longer int(S * long / short).  CenterCrop (functional.center_crop):
    top = int(round((new_h - S) / 2.0)), left likewise, Python's round (half to even)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(S * long / short)
    dst_w, dst_h = (S, new_long) if W <= H else (new_long, S)
    return dst_h, dst_w, int(round((dst_h - S) / 2.0)), int(round((dst_w - S) / 2.0))


def clean_caption(text):
    return CLEAN.sub("", str(text)).strip()


def permutation(n, seed):
    """The row order of pandas' df.sample(frac=1, random_state=seed)."""
    return np.random.RandomState(seed).permutation(n).tolist()


def read_pairs(root):
    """-> [(caption, image path)] of the datasets present under root, medpix first, cleaned and filtered as the reference does."""
    folders = [os.path.join(root, d, "images") for d in DATASETS]
    rows, found = [], 0
    for d in DATASETS:
        path = os.path.join(root, d, f"{d}.csv")
        if not os.path.exists(path):
            continue
        found += 1
        with open(path, newline="", encoding="utf-8") as f:
            rows += [(r.get(CAPTION_KEY), r.get(IMAGE_KEY)) for r in csv.DictReader(f)]
    if not found:
        raise RuntimeError(f"--finetune_root {root}: neither {DATASETS[0]}/{DATASETS[0]}.csv nor {DATASETS[1]}/{DATASETS[1]}.csv is there")
    logging.info(f"Loaded {len(rows)} samples from MedPix and PMC-CURD datasets")
    rows = [(clean_caption("nan" if c is None else c), fn) for c, fn in rows]          # (pandas reads an empty cell as NaN, and str(NaN) is "nan")
    rows = [(c, fn) for c, fn in rows if len(c) > MIN_CAPTION]
    logging.info(f"After caption filtering: {len(rows)} samples")
    pairs = []
    for caption, filename in rows:
        name = os.path.basename(filename or "")
        path = next((p for p in (os.path.join(d, name) for d in folders) if name and os.path.exists(p)), None)
        if path is None:
            logging.warning(f"Image {name} not found in any path during initialization")
            continue
        pairs.append((caption, path))
    return pairs


def split_pairs(pairs, seed):
    order = permutation(len(pairs), seed)
    cut = int(len(pairs) * 0.9)
    return [pairs[i] for i in order[:cut]], [pairs[i] for i in order[cut:]]


class CaptionPairs(Dataset):
    """sample = (pixels uint8 [H, W] or [H, W, 3], (dst_h, dst_w, y0, x0), caption)."""

    def __init__(self, pairs, img_size):
        self.pairs, self.S = list(pairs), int(img_size)
        if not MIN_SIZE <= self.S <= MAX_SIZE:
            raise RuntimeError(f"--finetune_root: --img_size {img_size} is outside the resize kernel's limits ({MIN_SIZE} .. {MAX_SIZE})")
        self.limit = image_limit(self.S)

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        Image = _pil()
        caption, path = self.pairs[i]
        S = self.S
        with Image.open(path) as im:
            if im.mode not in ("L", "RGB"):
                im = im.convert("RGB")
            W, H = im.size
            geom = geometry(W, H, S)
            channels = 1 if im.mode == "L" else 3
            if max(ksize_of(W, geom[1]), ksize_of(H, geom[0])) > MAX_KSIZE or W * H * channels > self.limit or max(geom[:2]) > MAX_DST:
                im = im.resize((geom[1], geom[0]), Image.BICUBIC)          # what the kernel would have made, byte for byte
                if geom[0] * geom[1] * channels > self.limit:
                    im = im.crop((geom[3], geom[2], geom[3] + S, geom[2] + S))
                    geom = (S, S, 0, 0)
            px = np.asarray(im)
        return px, geom, caption


class EpochBatches:
    """The loader's batch sampler: RankShardSampler's order cut into batches, and `stop()`: the iteration in flight yields nothing more, so that an
    abandoned epoch costs only the batches already handed to the workers."""

    def __init__(self, n, batch, shuffle, drop_last, rank=0, world=1, seed=0):
        self.sampler = RankShardSampler(n, rank, world, shuffle=shuffle, seed=seed, drop_last=drop_last and world > 1)
        self.batch, self.drop_last = int(batch), drop_last
        self._stopped = False

    def set_epoch(self, epoch):
        self.sampler.set_epoch(epoch)

    def stop(self):
        self._stopped = True

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch if self.drop_last else (n + self.batch - 1) // self.batch

    def __iter__(self):
        self._stopped = False
        idx = self.sampler.indices()
        for k in range(len(self)):
            if self._stopped:
                return
            yield idx[k * self.batch:(k + 1) * self.batch]


class ByteSlotRing:
    """The loader's collate_fn.  `slots` slots in SHARED memory, each `batch * limit` bytes, a descriptor int32 [batch, 8] and token ids int64
    [batch, ids_len], allocated once (before the workers are forked); a collate takes a free slot, writes into it and returns (MARK, slot, B,
    bytes, captions).  Word 3 of a descriptor row is the image's channel count (uia_resize_batch_rgb's form)."""

    MARK = "__uia_byte_ring__"

    def __init__(self, slots, batch, limit, ids_len, tokenizer):
        import multiprocessing as mp
        self.data = torch.empty((slots, batch * limit), dtype=torch.uint8).share_memory_()
        self.desc = torch.zeros((slots, batch, DESC), dtype=torch.int32).share_memory_()
        self.ids = torch.zeros((slots, batch, max(1, ids_len)), dtype=torch.int64).share_memory_()
        self.free = mp.get_context("fork").Queue()
        for i in range(slots):
            self.free.put(i)
        self.slots, self.batch, self.limit, self.tokenizer, self.pinned = slots, batch, limit, tokenizer, None

    def __call__(self, samples):
        slot = self.free.get()
        flat, desc, at = self.data[slot].numpy(), self.desc[slot].numpy(), 0
        for b, (px, geom, _) in enumerate(samples):
            H, W = px.shape[:2]
            flat[at:at + px.size] = px.reshape(-1)
            desc[b] = (at, H, W, 1 if px.ndim == 2 else 3, *geom)
            at += px.size
        texts = [s[2] for s in samples]
        if self.tokenizer is not None:
            self.ids[slot, :len(samples)].copy_(self.tokenizer(texts))
        return self.MARK, slot, len(samples), at, texts

    def release(self, slot):
        self.free.put(slot)

    def drain(self, loader, it):
        """An iteration that is abandoned: stop the loader's batch sampler and take the batches already in flight, so that their slots come back (the
        next iter() of a persistent-worker loader would throw them away with the slots they name)."""
        loader.batch_sampler.stop()
        for item in it:
            self.release(item[1])

    def pin(self):
        """hipHostRegister the ring, once, from the process that owns the GPU.  False when the runtime refuses: the prefetcher then stages."""
        if self.pinned is None:
            ok = True
            try:
                for t in (self.data, self.desc, self.ids):
                    ok = ok and int(torch.cuda.cudart().cudaHostRegister(t.data_ptr(), t.numel() * t.element_size(), 0)) == 0
                ok = ok and bool(self.data.is_pinned())
            except (AttributeError, RuntimeError):
                ok = False
            self.pinned = ok
        return self.pinned

    def unpin(self):
        """hipHostUnregister (DataModule.shutdown): a registration must not outlive the mapping it names."""
        if self.pinned:
            try:
                torch.cuda.synchronize()
                for t in (self.data, self.desc, self.ids):
                    torch.cuda.cudart().cudaHostUnregister(t.data_ptr())
            except (AttributeError, RuntimeError):
                pass
        self.pinned = None


def ring_slots(nw):
    """Every batch the workers may have in flight (prefetch_factor 2 each), the prefetcher's queue and hand (3), the consumer's batch and the one
    behind its event (2), and one to spare."""
    return 2 * nw + 6


class DataModule:
    """src/datasets/finetune.DataModule's interface over the caption folders.  Train: shuffle, drop_last; validation: neither.  Ranks take
    RankShardSampler's shards."""

    def __init__(self, args, rank=0, world=1, tokenizer=None):
        self.args, self.rank, self.world, self.tokenizer = args, rank, world, tokenizer
        train, val = split_pairs(read_pairs(args.finetune_root), args.seed)
        logging.info(f"Train samples: {len(train)}, Val samples: {len(val)}")
        self.train, self.val = CaptionPairs(train, args.img_size), CaptionPairs(val, args.img_size)
        self.train_sampler = None
        self._loaders = []

    def _loader(self, ds, train):
        a = self.args
        nw = max(0, min(int(getattr(a, "num_workers", 0) or 0), MAX_WORKERS if train else 2))
        if nw and torch.cuda.is_initialized():                  # never fork after the GPU is up
            logging.info("loader: the GPU is already initialised in this process; decoding in-process (num_workers=0)")
            nw = 0
        ids_len = int(self.tokenizer(["x"]).shape[1]) if self.tokenizer is not None else 0
        per_slot = a.batch_size * (ds.limit + DESC * 4 + ids_len * 8)
        slots = ring_slots(0)
        if nw:
            import shutil
            planned = getattr(self, "_shm_planned", 0)
            try:
                room = shutil.disk_usage("/dev/shm").free // 2 - planned
            except OSError:
                room = 0
            while nw > 0 and ring_slots(nw) * per_slot > room:  # (plan_workers' rule with this ring's slot count)
                nw -= 1
            slots = ring_slots(nw)
            if nw:
                self._shm_planned = planned + slots * per_slot
        sampler = EpochBatches(len(ds), a.batch_size, shuffle=train, drop_last=train, rank=self.rank, world=self.world, seed=getattr(a, "seed", 0))
        kw = dict(num_workers=nw, collate_fn=ByteSlotRing(slots, a.batch_size, ds.limit, ids_len, self.tokenizer))
        if nw:
            kw.update(persistent_workers=True, prefetch_factor=2)
        loader = DataLoader(ds, batch_sampler=sampler, **kw)
        if train:
            self.train_sampler = sampler
        self._loaders.append(loader)
        return loader

    def train_dataloader(self):
        return self._loader(self.train, True)

    def val_dataloader(self):
        return self._loader(self.val, False)

    def start_workers(self):
        """Fork the workers now, before the process touches the GPU; the consumer's first epoch takes this iterator."""
        for loader in self._loaders:
            if loader.num_workers > 0 and len(loader) > 0:
                loader._uia_first_iter = iter(loader)

    def set_epoch(self, epoch):
        if self.train_sampler is not None:
            self.train_sampler.set_epoch(epoch)

    def shutdown(self):
        for loader in self._loaders:
            loader.collate_fn.unpin()
            it = getattr(loader, "_iterator", None) or loader.__dict__.pop("_uia_first_iter", None)
            if it is not None and hasattr(it, "_shutdown_workers"):
                it._shutdown_workers()
            loader._iterator = None


class RaggedBatch:
    """What CaptionPrefetcher yields in the images' place: the device bytes and the host descriptor (a view of the ring's slot) of one batch."""

    def __init__(self, data, desc):
        self.data, self.desc = data, desc


class CaptionPrefetcher:
    """engine.DevicePrefetcher's interface — `for batch, tokens, ready in pf`, `wait_s`, `len`, `close()` — over a ByteSlotRing loader: a background
    thread copies a slot's bytes and token ids to the device on a copy stream (straight from the slot when the ring is pinned, else through pinned
    staging buffers); `batch` is a RaggedBatch for RgbResizeStage.  The descriptor is read from the slot by the stage's launch, so a slot goes back
    to the workers only behind the event the consumer's stream records when it asks for the next batch; before the consumer blocks on an empty
    queue it waits for those events, so the workers never starve for slots the consumer holds."""

    def __init__(self, loader, device, depth=2):
        self.loader, self.ring, self.device, self.depth = loader, loader.collate_fn, torch.device(device), max(1, depth)
        self.wait_s = 0.0
        self._dev = [None] * (self.depth + 2)
        self._copy = torch.cuda.Stream(device=self.device)
        self._stop = threading.Event()
        self._live = None
        self._held = []                                         # (consumer's event, ring slot)
        self._cur = None                                        # (device slot, ring slot) of the batch the consumer is working on

    def __len__(self):
        return len(self.loader)

    def _dev_slot(self, k, nbytes, dma):
        s = self._dev[k]
        if s is not None and s["free"] is not None:
            s["free"].synchronize()                             # the consumer's last reader of this device slot
        if s is None or s["d"].numel() < nbytes:
            cap = max(nbytes + nbytes // 4, 1 << 16)
            s = {"d": torch.empty(cap, dtype=torch.uint8, device=self.device),
                 "d_ids": torch.empty(self.ring.ids.shape[1:], dtype=torch.int64, device=self.device), "free": None, "copied": None,
                 "h": None if dma else torch.empty(cap, dtype=torch.uint8, pin_memory=True),
                 "h_ids": None if dma else torch.empty(self.ring.ids.shape[1:], dtype=torch.int64, pin_memory=True)}
            self._dev[k] = s
        return s

    def _producer(self, it, q):
        ring = self.ring
        try:
            torch.cuda.set_device(self.device)
            dma = ring.pin()
            k = 0
            for _mark, slot, B, nbytes, _texts in it:
                s = self._dev_slot(k % len(self._dev), nbytes, dma)
                k += 1
                src, src_ids = ring.data[slot, :nbytes], ring.ids[slot, :B]
                if not dma:
                    if s["copied"] is not None:
                        s["copied"].synchronize()
                    s["h"][:nbytes].copy_(src)
                    s["h_ids"][:B].copy_(src_ids)
                    src, src_ids = s["h"][:nbytes], s["h_ids"][:B]
                with torch.cuda.stream(self._copy):
                    s["d"][:nbytes].copy_(src, non_blocking=True)
                    s["d_ids"][:B].copy_(src_ids, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self._copy)
                s["copied"] = ev
                if not self._put(q, (s, slot, RaggedBatch(s["d"][:nbytes], ring.desc[slot, :B]), s["d_ids"][:B], ev)):
                    ev.synchronize()
                    ring.release(slot)
                    break
            else:
                self._put(q, None)
                return
            ring.drain(self.loader, it)                         # close(): the batches the loader had in flight
        except BaseException as e:                              # surfaces in the consumer
            self._put(q, e)

    def _put(self, q, item):
        while not self._stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def _done_with_current(self):
        """Everything that reads the consumer's batch (its descriptor copy included) is enqueued: its slots are free behind an event recorded now."""
        cur, self._cur = self._cur, None
        if cur is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            cur[0]["free"] = ev
            self._held.append((ev, cur[1]))

    def _release_held(self, wait):
        while self._held and (wait or self._held[0][0].query()):
            ev, slot = self._held.pop(0)
            ev.synchronize()
            self.ring.release(slot)

    def close(self):
        """Stops the iteration in flight: the producer drains what the loader had prefetched, every slot in the queue or behind an event goes back."""
        live, self._live = self._live, None
        if live is not None:
            th, q = live
            self._stop.set()
            while th.is_alive() or not q.empty():
                try:
                    item = q.get(timeout=0.05)
                    if isinstance(item, tuple):
                        item[4].synchronize()
                        self.ring.release(item[1])
                except queue.Empty:
                    pass
                th.join(timeout=0.05)
            self._stop.clear()
        self._done_with_current()
        self._release_held(wait=True)

    def __iter__(self):
        q = queue.Queue(maxsize=self.depth)
        first = self.loader.__dict__.pop("_uia_first_iter", None)
        self.close()
        th = threading.Thread(target=self._producer, args=(first if first is not None else iter(self.loader), q), daemon=True)
        th.start()
        self._live = (th, q)
        return self._consume(th, q)

    def _consume(self, th, q):
        while True:
            self._done_with_current()                           # recorded BEFORE the queue frees a place: the producer cannot reach this slot until then
            t0 = time.perf_counter()
            self._release_held(wait=False)
            try:
                item = q.get_nowait()
            except queue.Empty:
                self._release_held(wait=True)                   # about to stand still: hold no slot a worker may be waiting for
                item = q.get()
            self.wait_s += time.perf_counter() - t0
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            s, slot, batch, tokens, ev = item
            self._cur = (s, slot)
            yield batch, tokens, ev
        th.join()
        self._release_held(wait=True)
        if self._live is not None and self._live[0] is th:
            self._live = None


class RgbResizeStage:
    """`images = stage(batch)` behind the prefetcher's event: one uia_resize_batch_rgb launch on the current stream -> fp32 [B, 3, S, S] in [0, 1],
    the reference's Resize + CenterCrop + ToTensor.  Output and workspace are allocated once per batch size (the last validation batch is smaller)."""

    def __init__(self, img_size):
        self.S = int(img_size)
        self._bufs = {}

    def __call__(self, batch):
        from uia_hip import ops
        B = batch.desc.shape[0]
        if B not in self._bufs:
            dev = batch.data.device
            self._bufs[B] = (torch.empty(B, 3, self.S, self.S, dtype=torch.float32, device=dev), ops.resize_workspace(B, dev))
        out, ws = self._bufs[B]
        return ops.resize_batch_rgb(batch.data, batch.desc, self.S, out, ws)
