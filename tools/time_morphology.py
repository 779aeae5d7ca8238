"""The cost of uia_mask_morphology (reported in DESIGN.md §4 "Prediction: morphology") beside the per-mask host loop it replaces.

  call:   ops.mask_morphology on a batch of --batch masks of 480 x 640 with their overlays — three blobs with holes plus speckle, what a segmentation
          model predicts on ultrasound — at three settings (r_close, r_open, fill): (3, 2, -1), the everyday one; (16, 0, 0), a closing alone; (64, 64,
          -1), the largest radii the kernel takes.  HIP events around one call (descriptor copy and every launch of the call), the median of --reps
          calls after --warmup.  The call works in place, so the buffer is restored from a device copy before every call, outside the events.
  host:   the loop a user writes today: per mask one .cpu(), then scipy.ndimage's binary_closing / binary_fill_holes / binary_opening with the disk and
          the kernel's border values (a dilation sees nothing outside the image, an erosion is not eaten from outside); a host clock around the whole
          batch, one pass after one warm-up mask, and whether its masks equal the kernel's.  Said so when scipy does not import.

Prints one JSON line, with the device's clock and power as rocm-smi reports them right after the timed calls."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

SETTINGS = ((3, 2, -1), (16, 0, 0), (64, 64, -1))


def device_state():
    """Clock and power as rocm-smi reports them (read only); what could not be read is said so."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower() or "power" in k.lower()}
    except Exception as e:                                       # the figure is context, not a result
        return {"not_read": repr(e)}


def blobs_with_holes(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = rng.random((H, W)) < 0.004                               # speckle
    for _ in range(3):
        cy, cx, ry, rx = rng.integers(60, H - 60), rng.integers(80, W - 80), rng.integers(20, 90), rng.integers(30, 120)
        d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        m |= d <= 1.0
        m &= ~(((yy - cy) / (0.3 * ry)) ** 2 + ((xx - cx - 0.3 * rx) / (0.3 * rx)) ** 2 <= 1.0)       # a hole ...
        m &= ~((np.abs(yy - cy) <= 1) & (xx > cx) & (d <= 1.2))                                       # ... and a broken rim
    m &= rng.random((H, W)) >= 0.002                             # pin-holes
    return (m * 255).astype(np.uint8)


def timed(fn, restore, warmup, reps):
    for _ in range(warmup):
        restore()
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"ms": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r * r


def host_morphology(mask, r_close, r_open, fill, eight):
    """What the call does to one mask, with scipy on the host -> the set after."""
    from scipy import ndimage
    x = mask != 0
    if r_close:
        x = ndimage.binary_erosion(ndimage.binary_dilation(x, disk(r_close), border_value=0), disk(r_close), border_value=1)
    if fill:                                                     # (the tool's settings fill holes of any size)
        x = ndimage.binary_fill_holes(x, np.ones((3, 3), bool) if eight else None)
    if r_open:
        x = ndimage.binary_dilation(ndimage.binary_erosion(x, disk(r_open), border_value=1), disk(r_open), border_value=0)
    return x


def time_batch(args, setting):
    from uia_hip import ops
    from src.utils.viz import NativeMaskWriter
    dev = torch.device("cuda:0")
    B, H, W = args.batch, 480, 640
    r_close, r_open, fill = setting
    conn = 4                                                     # the holes of an 8-connected foreground
    rng = np.random.default_rng(0)
    where, total = NativeMaskWriter.layout([(H, W)] * B, overlay=True)
    host = np.zeros(total, dtype=np.uint8)
    for moff, ooff in where:
        m, g = blobs_with_holes(rng, H, W), rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        host[moff:moff + H * W] = m.ravel()
        host[ooff:ooff + 3 * H * W] = np.stack([g, np.maximum(g, m), g], axis=-1).ravel()
    orig = torch.from_numpy(host).to(dev)
    buf = orig.clone()
    desc = torch.tensor([[moff, H, W, ooff, r_close, r_open, fill, conn] for moff, ooff in where], dtype=torch.int32).pin_memory()
    res = {"batch": B, "H": H, "W": W, "r_close": r_close, "r_open": r_open, "fill_holes": fill, "hole_connectivity": conn,
           "workspace_bytes": int(ops.mask_morphology_workspace(B, B * H * W, dev).numel())}
    res.update(timed(lambda: ops.mask_morphology(buf, desc), lambda: buf.copy_(orig), args.warmup, args.reps))
    res["device"] = device_state()
    stats = ops.mask_morphology(buf.copy_(orig), desc).cpu().numpy()
    flat = buf.cpu().numpy()
    res["added_per_mask"], res["removed_per_mask"] = round(float(stats[:, 5].mean()), 1), round(float(stats[:, 6].mean()), 1)
    try:
        import scipy  # noqa: F401
    except ImportError:
        res["host_loop"] = "not run: scipy does not import here"
        return res
    n = B if args.host_masks <= 0 or max(r_close, r_open) <= 16 else min(B, args.host_masks)
    host_morphology(orig[:H * W].cpu().numpy().reshape(H, W), r_close, r_open, fill, False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [host_morphology(orig[moff:moff + H * W].cpu().numpy().reshape(H, W), r_close, r_open, fill, False) for moff, _ in where[:n]]
    res["host_loop_ms"] = round((time.perf_counter() - t0) * 1e3 * B / n, 1)
    res["host_loop_masks_timed"] = n
    res["masks_equal"] = all(np.array_equal(flat[moff:moff + H * W].reshape(H, W) != 0, x) for (moff, _), x in zip(where, out))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--host_masks", type=int, default=0, help="at radii above 16, where scipy needs many seconds a mask, time the host loop on the first N masks only "
                   "and scale to the batch (0: all of them)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_morphology.py measures on the MI355X: no GPU here, nothing measured")
    print(json.dumps({f"close{rc}_open{ro}_fill{f}": time_batch(args, (rc, ro, f)) for rc, ro, f in SETTINGS}))


if __name__ == "__main__":
    main()
