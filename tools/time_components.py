"""The cost of uia_mask_components (reported in DESIGN.md §4 "Prediction: components") beside the per-mask host loop it replaces.

  call:   ops.mask_components on a batch of --batch masks of 480 x 640 with their overlays, min_area 50, the 3 largest kept, 4 list rows: HIP
          events around one call (descriptor copy and every launch of the call), the median of --reps calls after --warmup.  The call works in place, so the
          buffer is restored from a device copy before every call, outside the events.  Two contents: a few large blobs plus speckle (what a
          segmentation model predicts; 8-connected), and uniform noise at 50 % (4-connected: some 20 000 components a mask, the most union, atomic and
          selection work).
  host:   the loop a user writes today: per mask one .cpu(), scipy.ndimage.label, areas with numpy, the same filter, a box and a centre per kept
          component; a host clock around the whole batch, the median of three passes, and whether its masks equal the kernel's.  Said so when scipy does
          not import.
  worst:  one 4096 x 4096 mask of 50 % noise, 4-connected, the 32 largest kept and listed: the most components one image can bring to the selection.

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


def device_state():
    """Clock and power as rocm-smi reports them (read only); what could not be read is said so."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower() or "power" in k.lower()}
    except Exception as e:                                       # the figure is context, not a result
        return {"not_read": repr(e)}


def blobs(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = rng.random((H, W)) < 0.004                               # speckle
    for _ in range(3):
        cy, cx, ry, rx = rng.integers(60, H - 60), rng.integers(80, W - 80), rng.integers(20, 90), rng.integers(30, 120)
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return (m * 255).astype(np.uint8)


def noise(rng, H, W):
    return ((rng.random((H, W)) < 0.5) * 255).astype(np.uint8)


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


def host_filter(mask, min_area, keep, eight, rows):
    """What the call does to one mask, with scipy and numpy on the host -> (mask after, [(area, ymin, xmin, ymax, xmax, cy, cx)])."""
    from scipy import ndimage
    labels, n = ndimage.label(mask != 0, structure=np.ones((3, 3), int) if eight else None)
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    order = np.argsort(-area, kind="stable")                     # scipy numbers components by their first pixel
    kept = order[area[order] >= min_area][:keep if keep > 0 else None]
    out = np.where(np.isin(labels, kept + 1), mask, 0).astype(np.uint8)
    found = ndimage.find_objects(labels)
    lesions = []
    for i in kept[:rows]:
        sl = found[i]
        ys, xs = np.nonzero(labels[sl] == i + 1)
        lesions.append((int(area[i]), sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1, int(ys.sum() + sl[0].start * ys.size) // int(area[i]),
                        int(xs.sum() + sl[1].start * xs.size) // int(area[i])))
    return out, lesions


def time_batch(args, content, make, conn):
    from uia_hip import ops
    from src.utils.viz import NativeMaskWriter
    dev = torch.device("cuda:0")
    B, H, W = args.batch, 480, 640
    min_area, keep, rows = 50, 3, 4
    rng = np.random.default_rng(0)
    where, total = NativeMaskWriter.layout([(H, W)] * B, overlay=True)
    host = np.zeros(total, dtype=np.uint8)
    for moff, ooff in where:
        m, g = make(rng, H, W), rng.integers(0, 256, size=(H, W), dtype=np.uint8)
        host[moff:moff + H * W] = m.ravel()
        host[ooff:ooff + 3 * H * W] = np.stack([g, np.maximum(g, m), g], axis=-1).ravel()
    orig = torch.from_numpy(host).to(dev)
    buf = orig.clone()
    desc = torch.tensor([[moff, H, W, ooff, min_area, keep, conn, 0] for moff, ooff in where], dtype=torch.int32).pin_memory()
    res = {"content": content, "batch": B, "H": H, "W": W, "min_area": min_area, "keep": keep, "connectivity": conn, "max_list": rows}
    res.update(timed(lambda: ops.mask_components(buf, desc, rows), lambda: buf.copy_(orig), args.warmup, args.reps))
    res["device"] = device_state()
    stats, lst = ops.mask_components(buf.copy_(orig), desc, rows)
    stats, lst, flat = stats.cpu().numpy(), lst.cpu().numpy(), buf.cpu().numpy()
    res["components_found_per_mask"] = round(float(stats[:, 5].mean()), 1)
    try:
        import scipy  # noqa: F401
    except ImportError:
        res["host_loop"] = "not run: scipy does not import here"
        return res

    def host_loop():
        return [host_filter(orig[moff:moff + H * W].cpu().numpy().reshape(H, W), min_area, keep, conn == 8, rows) for moff, _ in where]
    host_loop()
    took = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = host_loop()
        took.append((time.perf_counter() - t0) * 1e3)
    res["host_loop_ms"] = round(statistics.median(took), 2)
    res["masks_equal"] = all(np.array_equal(flat[moff:moff + H * W].reshape(H, W), m) for (moff, _), (m, _) in zip(where, out))
    res["lists_equal"] = all([tuple(int(v) for v in r[[0, 1, 2, 3, 4, 6, 7]]) for r in rows_b if r[0] > 0] == les for rows_b, (_, les) in zip(lst, out))
    return res


def time_worst(args):
    from uia_hip import ops
    dev = torch.device("cuda:0")
    N = 4096
    orig = torch.from_numpy(noise(np.random.default_rng(1), N, N).ravel()).to(dev)
    buf = orig.clone()
    desc = torch.tensor([[0, N, N, -1, 2, 32, 4, 0]], dtype=torch.int32).pin_memory()
    res = {"content": "noise 50 %", "H": N, "W": N, "min_area": 2, "keep": 32, "connectivity": 4, "max_list": 32}
    res.update(timed(lambda: ops.mask_components(buf, desc, 32), lambda: buf.copy_(orig), args.warmup, max(5, args.reps // 5)))
    stats, _ = ops.mask_components(buf.copy_(orig), desc, 32)
    res["components_found"] = int(stats[0, 5])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_components.py measures on the MI355X: no GPU here, nothing measured")
    print(json.dumps({"blobs": time_batch(args, "three blobs plus 0.4 % speckle", blobs, 8), "noise": time_batch(args, "noise 50 %", noise, 4), "worst": time_worst(args)}))


if __name__ == "__main__":
    main()
