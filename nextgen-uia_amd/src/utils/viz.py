"""The pictures of the segmentation test pass — what the reference's visualize_seg (src/utils/tools.py:278-315) writes with numpy and PIL, one image at a
time on the host: per test image `<stem>.png` (ground truth red, prediction green), `<stem>_overlay.png` (the same over the grey input) and
`<stem>_pred.png` (the binary mask).

Here the pixels of a whole batch come from one launch (`uia_hip.ops.seg_viz`, csrc/seg_viz.hip) on the stream the evaluation runs on, with the arg-max
rule of the Dice / IoU / surface metrics, so a written mask is the mask the metrics were computed on.  `SegVisualizer.submit` enqueues that launch and the
three device-to-host copies behind it into a pinned slot, records an event and hands (event, slot, names) to a small pool of writer threads; a writer
waits on the event, adds the PNG filter bytes, compresses (zlib releases the interpreter lock) and writes.  The evaluation loop never waits for the
device; it waits for a writer only when every pinned slot is still being written.

`write_png` is the whole encoder: 8-bit grey or RGB, one IDAT, filter type 0 on every row, from zlib and struct alone (PIL is not part of the build image).
"""
import queue
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
# zlib level of the written files.  Measured on the UNet baseline's test pass (the fastest of the segmentation entries; DESIGN.md §4 "Segmentation
# visualisation"): at level 1 the four writers keep up with the pass, at zlib's default 6 they need 3.5 times as long per file and test() waits for them;
# the files are 3 % larger.
PNG_LEVEL = 1
MAX_WRITERS = 4


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(array, level=PNG_LEVEL):
    """uint8 [H, W] (grey) or [H, W, 3] (RGB) -> the bytes of a PNG file."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: a uint8 array [H, W] or [H, W, 3] is required, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.empty((h, 1 + a.size // h), dtype=np.uint8)
    rows[:, 0] = 0                                               # filter type 0 (None) on every row
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)      # bit depth 8, colour type grey / RGB, deflate, adaptive filtering, no interlace
    return PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, array, level=PNG_LEVEL):
    if isinstance(array, torch.Tensor):
        array = array.detach().cpu().numpy()
    data = encode_png(array, level)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def png_names(name):
    """The three file names of one sample, as the reference forms them (tools.py:303-315)."""
    stem = str(Path(name).stem)
    return f"{stem}.png", f"{stem}_overlay.png", f"{stem}_pred.png"


class SegVisualizer:
    def __init__(self, viz_path, max_batch, size, workers=MAX_WRITERS, level=PNG_LEVEL, device=None):
        self.viz_path, self.max_batch, self.size, self.level = str(viz_path), int(max_batch), int(size), level
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        B, S = self.max_batch, self.size
        self._mask, self._overlay = (torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.device) for _ in range(2))
        self._pred = torch.empty(B, S, S, dtype=torch.uint8, device=self.device)
        workers = max(1, min(int(workers), MAX_WRITERS))
        self._free = queue.Queue()
        for _ in range(workers + 2):                             # one slot per writer and two being filled: a slot goes back only after its files are written
            self._free.put(tuple(torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (self._mask, self._overlay, self._pred)))
        self._pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="seg-viz")
        self._jobs = []
        self.files = self.bytes = 0
        self.encode_s = 0.0

    def submit(self, images, labels, preds, names):
        """images fp32 [n, 1|3, S, S], labels uint8 / fp32 [n, 1, S, S], preds fp32 logits [n, 2, S, S] on the device, n <= max_batch, and n file names.
        Enqueues on the current stream and returns; the files appear behind it."""
        from uia_hip import ops
        n = len(names)
        if not (0 < n <= self.max_batch and images.shape[0] == n and labels.shape[0] == n and preds.shape[0] == n):
            raise ValueError(f"SegVisualizer.submit: {n} names for batches of {images.shape[0]} / {labels.shape[0]} / {preds.shape[0]} (at most {self.max_batch})")
        if tuple(preds.shape[2:]) != (self.size, self.size):
            raise ValueError(f"SegVisualizer.submit: predictions of {tuple(preds.shape[2:])}, built for {self.size} x {self.size}")
        self._reap()
        if labels.dtype not in (torch.uint8, torch.float32):
            labels = labels.float()
        dev = (self._mask[:n], self._overlay[:n], self._pred[:n])
        ops.seg_viz(preds.detach().float().contiguous(), images.detach().float().contiguous(), labels.detach().contiguous(), *dev)
        slot = self._free.get()
        for h, d in zip(slot, dev):
            h[:n].copy_(d, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._jobs.append(self._pool.submit(self._write, done, slot, list(names)))

    def _write(self, done, slot, names):
        import time
        try:
            done.synchronize()
            t0 = time.perf_counter()
            size = 0
            for i, name in enumerate(names):
                for file_name, plane in zip(png_names(name), slot):
                    size += write_png(f"{self.viz_path}/{file_name}", plane[i].numpy(), self.level)
            return 3 * len(names), size, time.perf_counter() - t0
        finally:
            self._free.put(slot)

    def _reap(self, wait=False):
        """Collects finished jobs; a writer's exception surfaces here."""
        keep = []
        for job in self._jobs:
            if wait or job.done():
                files, size, seconds = job.result()
                self.files, self.bytes, self.encode_s = self.files + files, self.bytes + size, self.encode_s + seconds
            else:
                keep.append(job)
        self._jobs = keep

    def close(self):
        """Drains the writers; re-raises the first exception one of them met."""
        try:
            self._pool.shutdown(wait=True)
            self._reap(wait=True)
        finally:
            self._jobs = []


class NativeMaskWriter:
    """The files of src/models/predict.py: per image `masks/<stem>.png` (8-bit grey, the image's own H x W) and, with overlay=True, `overlays/<stem>.png`
    (RGB, the prediction in green over the grey input) under out_dir.  `submit` lays the batch's masks and overlays out back to back in one device
    buffer, enqueues ONE launch of `uia_hip.ops.seg_predict_native` with the batch's own ragged source bytes, one copy of that buffer and one of the
    statistics into a pinned slot, records an event and hands the slot to a writer thread (at most four), as SegVisualizer does.  The descriptor lives in
    the slot, which goes back only behind the event.  `close()` joins the writers, re-raises a writer's exception and returns the batches' (names,
    [(H, W)], stats int32 [n, 8]) in the order they were submitted.

    min_area / keep / connectivity / lesions: connected-component filtering on the device.  With all four at their defaults nothing else is enqueued.
    Otherwise ONE `uia_hip.ops.mask_components` call on the device buffer follows the launch, before the copies: components below min_area pixels and
    those beyond the `keep` largest (0 = any number) leave masks and overlays, the slot's stats are that call's (words 0-4 keep their meaning, 5-7 are
    components found, kept and the foreground before), and the first `lesions` (<= 32) kept components of every image are copied into the slot as well:
    `lesion_lists()` returns them after `close()`, int32 [n, lesions, 8] per batch in submission order.

    threshold / prob / spread, and `submit` with logits [K, n, 2, S, S] or with `flips`: the ensemble launch.  With a 4-D tensor, no flips and these three
    at their defaults `submit` makes the `seg_predict_native` call above and nothing else.  Otherwise it makes ONE `uia_hip.ops.seg_predict_native_ens`
    launch in its place: the mask is 255 where the members' mean foreground probability exceeds `threshold`; with prob=True `probs/<stem>.png` (8-bit grey,
    that mean) and with spread=True `spread/<stem>.png` (8-bit grey, the largest minus the smallest member) are written too, their planes lying behind the
    image's overlay in the buffer.  The slot then carries the launch's sums as well: `sums()` returns them after `close()`, int64 [n, 2] per batch in
    submission order (sum of the probability bytes over the launch's own mask, sum of the spread bytes over the image).  The component filter runs behind
    the launch as before and touches only masks and overlays.

    close_radius / open_radius / fill_holes: morphology on the device.  With all three at 0 nothing else is enqueued.  Otherwise ONE
    `uia_hip.ops.mask_morphology` call on the device buffer follows the mask launch (plain or ensemble), before the optional component call and before
    the copies: a closing with the disk of close_radius (0 .. 64), the holes of the result filled (fill_holes -1: every hole, N > 0: holes of at most N
    pixels; a hole is a background component under the connectivity 12 - `connectivity`, the complement of the foreground's), then an opening with the
    disk of open_radius.  The slot then carries the call's words 5-7 as well: `morphology_stats()` returns them after `close()`, int32 [n, 3] per batch
    in submission order (pixels added, pixels removed, foreground of the launch's own mask)."""

    def __init__(self, out_dir, overlay=True, workers=MAX_WRITERS, level=PNG_LEVEL, device=None, min_area=0, keep=0, connectivity=8, lesions=0, threshold=0.5,
                 prob=False, spread=False, close_radius=0, open_radius=0, fill_holes=0):
        self.out_dir, self.overlay, self.level = Path(out_dir), bool(overlay), level
        self.threshold, self.prob, self.spread = float(threshold), bool(prob), bool(spread)
        if not 0.0 < self.threshold < 1.0:
            raise ValueError(f"NativeMaskWriter: threshold={threshold} (0 < threshold < 1)")
        self.ensemble = (self.threshold, self.prob, self.spread) != (0.5, False, False)
        self._sums = {}
        self.min_area, self.keep, self.connectivity, self.lesions = int(min_area), int(keep), int(connectivity), int(lesions)
        if self.min_area < 0 or self.keep < 0 or self.connectivity not in (4, 8) or not 0 <= self.lesions <= 32:
            raise ValueError(f"NativeMaskWriter: min_area={min_area}, keep={keep} (>= 0), connectivity={connectivity} (4 or 8), lesions={lesions} (0 .. 32)")
        self.components = (self.min_area, self.keep, self.connectivity, self.lesions) != (0, 0, 8, 0)
        self._lists = {}
        self.close_radius, self.open_radius, self.fill_holes = int(close_radius), int(open_radius), int(fill_holes)
        if not 0 <= self.close_radius <= 64 or not 0 <= self.open_radius <= 64 or self.fill_holes < -1:
            raise ValueError(f"NativeMaskWriter: close_radius={close_radius}, open_radius={open_radius} (0 .. 64), fill_holes={fill_holes} (>= -1)")
        self.morphology = (self.close_radius, self.open_radius, self.fill_holes) != (0, 0, 0)
        self._morph = {}
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        (self.out_dir / "masks").mkdir(parents=True, exist_ok=True)
        if self.overlay:
            (self.out_dir / "overlays").mkdir(parents=True, exist_ok=True)
        if self.prob:
            (self.out_dir / "probs").mkdir(parents=True, exist_ok=True)
        if self.spread:
            (self.out_dir / "spread").mkdir(parents=True, exist_ok=True)
        workers = max(1, min(int(workers), MAX_WRITERS))
        self._free = queue.Queue()
        for _ in range(workers + 2):
            self._free.put({"desc": None, "out": None, "stats": None, "cdesc": None, "list": None, "sums": None, "mdesc": None, "morph": None})
        self._dev_out = None
        self._pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="native-mask")
        self._jobs, self._done = [], {}
        self.files = self.bytes = self.batches = 0

    @staticmethod
    def layout(sizes, overlay, prob=False, spread=False):
        """[(H, W)] -> ([(mask offset, overlay offset or -1)], total bytes): every image's mask, then its overlay, back to back.  With prob or spread the
        image's probability plane and then its spread plane lie behind its overlay, and the rows are (mask, overlay or -1, probability or -1, spread or
        -1) offsets."""
        at, where = 0, []
        for H, W in sizes:
            moff, at = at, at + H * W
            ooff = poff = roff = -1
            if overlay:
                ooff, at = at, at + 3 * H * W
            if prob:
                poff, at = at, at + H * W
            if spread:
                roff, at = at, at + H * W
            where.append((moff, ooff, poff, roff) if prob or spread else (moff, ooff))
        return where, at

    def submit(self, logits, batch, names, flips=None):
        """logits fp32 [n, 2, S, S] on the device, batch the folder.RaggedBatch the logits were computed from (its descriptor carries every image's
        offset, H and W), n file names.  Enqueues on the current stream and returns; the files appear behind it.  An ensemble: logits [K, n, 2, S, S] and
        flips, K values 0 .. 3 (bit 0: the member saw the horizontally flipped input, bit 1: the vertically flipped one; None: no member did)."""
        from uia_hip import ops
        n = len(names)
        members = logits.dim() == 5
        if not (n > 0 and logits.shape[1 if members else 0] == n and batch.desc.shape[0] == n):
            raise ValueError(f"NativeMaskWriter.submit: {n} names for {logits.shape[1 if members else 0]} predictions of {batch.desc.shape[0]} images")
        ens = members or flips is not None or self.ensemble
        self._reap()
        geo = batch.desc[:, :3].tolist()
        sizes = [(H, W) for _, H, W in geo]
        where, total = self.layout(sizes, self.overlay, self.prob, self.spread)
        where = [(w + (-1, -1))[:4] for w in where]
        slot = self._free.get()
        if slot["desc"] is None or slot["desc"].shape[0] < n:
            slot["desc"] = torch.empty(n, ops.SEG_NATIVE_DESC, dtype=torch.int32, pin_memory=True)
            slot["stats"] = torch.empty(n, ops.SEG_NATIVE_DESC, dtype=torch.int32, pin_memory=True)
        if slot["out"] is None or slot["out"].numel() < total:
            slot["out"] = torch.empty(total + total // 4, dtype=torch.uint8, pin_memory=True)
        if self._dev_out is None or self._dev_out.numel() < total:
            self._dev_out = torch.empty(total + total // 4, dtype=torch.uint8, device=self.device)
        desc = slot["desc"][:n]
        out = self._dev_out[:total]
        src = batch.data if self.overlay else None
        if not ens:
            desc.copy_(torch.tensor([[off if self.overlay else -1, H, W, moff, ooff, 0, 0, 0] for (off, H, W), (moff, ooff, _, _) in zip(geo, where)],
                                    dtype=torch.int32))
            stats = ops.seg_predict_native(logits.detach().float().contiguous(), src, desc, out)
        else:
            desc.copy_(torch.tensor([[off if self.overlay else -1, H, W, moff, ooff, poff, roff, 0] for (off, H, W), (moff, ooff, poff, roff) in zip(geo, where)],
                                    dtype=torch.int32))
            stack = (logits if members else logits.unsqueeze(0)).detach().float().contiguous()
            stats, sums = ops.seg_predict_native_ens(stack, [0] * stack.shape[0] if flips is None else flips, src, desc, out, threshold=self.threshold)
            if slot["sums"] is None or slot["sums"].shape[0] < n:
                slot["sums"] = torch.empty(n, 2, dtype=torch.int64, pin_memory=True)
            slot["sums"][:n].copy_(sums, non_blocking=True)
        if self.morphology:
            if slot["mdesc"] is None or slot["mdesc"].shape[0] < n:
                slot["mdesc"] = torch.empty(n, ops.MASK_MORPHOLOGY_DESC, dtype=torch.int32, pin_memory=True)
                slot["morph"] = torch.empty(n, 3, dtype=torch.int32, pin_memory=True)
            mdesc = slot["mdesc"][:n]
            mdesc.copy_(torch.tensor([[moff, H, W, ooff, self.close_radius, self.open_radius, self.fill_holes, 12 - self.connectivity]
                                      for (H, W), (moff, ooff, _, _) in zip(sizes, where)], dtype=torch.int32))
            stats = ops.mask_morphology(out, mdesc)
            slot["morph"][:n].copy_(stats[:, 5:8], non_blocking=True)
        if self.components:
            if slot["cdesc"] is None or slot["cdesc"].shape[0] < n:
                slot["cdesc"] = torch.empty(n, ops.MASK_COMPONENTS_DESC, dtype=torch.int32, pin_memory=True)
                slot["list"] = torch.empty(n, self.lesions, 8, dtype=torch.int32, pin_memory=True)
            cdesc = slot["cdesc"][:n]
            cdesc.copy_(torch.tensor([[moff, H, W, ooff, self.min_area, self.keep, self.connectivity, 0] for (H, W), (moff, ooff, _, _) in zip(sizes, where)],
                                     dtype=torch.int32))
            stats, rows = ops.mask_components(out, cdesc, self.lesions)
            slot["list"][:n].copy_(rows, non_blocking=True)
        slot["out"][:total].copy_(out, non_blocking=True)
        slot["stats"][:n].copy_(stats, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._jobs.append(self._pool.submit(self._write, self.batches, done, slot, list(names), sizes, where, ens))
        self.batches += 1

    def _write(self, k, done, slot, names, sizes, where, ens=False):
        try:
            done.synchronize()
            flat, size, files = slot["out"].numpy(), 0, 0
            for name, (H, W), (moff, ooff, poff, roff) in zip(names, sizes, where):
                stem = str(Path(name).stem)
                planes = [("masks", moff, (H, W)), ("overlays", ooff, (H, W, 3)), ("probs", poff, (H, W)), ("spread", roff, (H, W))]
                for folder, off, shape in planes:
                    if off >= 0:
                        size += write_png(self.out_dir / folder / f"{stem}.png", flat[off:off + int(np.prod(shape))].reshape(shape), self.level)
                        files += 1
            if self.components:
                self._lists[k] = slot["list"][:len(names)].clone().numpy()
            if ens:
                self._sums[k] = slot["sums"][:len(names)].clone().numpy()
            if self.morphology:
                self._morph[k] = slot["morph"][:len(names)].clone().numpy()
            return k, names, sizes, slot["stats"][:len(names)].clone().numpy(), files, size
        finally:
            self._free.put(slot)

    def _reap(self, wait=False):
        """Collects finished jobs; a writer's exception surfaces here."""
        keep = []
        for job in self._jobs:
            if wait or job.done():
                k, names, sizes, stats, files, size = job.result()
                self._done[k] = (names, sizes, stats)
                self.files, self.bytes = self.files + files, self.bytes + size
            else:
                keep.append(job)
        self._jobs = keep

    def close(self):
        """Joins the writers; re-raises the first exception one of them met; -> [(names, [(H, W)], stats)] in submission order."""
        try:
            self._pool.shutdown(wait=True)
            self._reap(wait=True)
        finally:
            self._jobs = []
        return [self._done[k] for k in sorted(self._done)]

    def lesion_lists(self):
        """After close(): per batch, in submission order, int32 [n, lesions, 8] — per image the first `lesions` kept components, largest first, as rows
        (area, ymin, xmin, ymax, xmax, first pixel, cy, cx), unused rows zero.  Empty when the writer filters nothing."""
        return [self._lists[k] for k in sorted(self._lists)]

    def sums(self):
        """After close(): per batch that went through the ensemble launch, in submission order, int64 [n, 2] — per image the sum of the probability bytes
        over the launch's own (unfiltered) mask and the sum of the spread bytes over the image.  Empty when no batch did."""
        return [self._sums[k] for k in sorted(self._sums)]

    def morphology_stats(self):
        """After close(): per batch, in submission order, int32 [n, 3] — per image (pixels the morphology added, pixels it removed, foreground of the
        launch's own mask before it).  Empty when the writer was built without close_radius, open_radius and fill_holes."""
        return [self._morph[k] for k in sorted(self._morph)]
