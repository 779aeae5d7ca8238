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
