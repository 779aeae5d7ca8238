"""The cost of uia_seg_predict_native_ens (reported in DESIGN.md §4 "Prediction: ensembles") beside the eager loop it replaces and beside its floor.

  launch: ops.seg_predict_native_ens on --batch 480 x 640 pictures under K members' S = 224 logits (flips 0, 1, 2, 3 in turn), all four outputs — masks,
          overlays, probability maps, spread maps — for K = 1, 4 and 12: HIP events around one call (the descriptor copy, the initial values and the
          kernel), the median of --reps calls after --warmup.
  bytes:  what the call has to move, counted from the shapes (every member's two logit planes once, every source byte once, every output byte once), and
          that over the launch time as a share of the HBM peak.
  eager:  the same outputs from the loop a user would write, all on the device: per member and picture torch.flip, F.interpolate and sigmoid of the
          difference, then mean, threshold, max - min, the two byte maps and the overlay; a host clock around the whole batch that ends in a
          synchronize, the median of three passes.
  floor:  K launches of ops.seg_predict_native on the same pictures, masks and overlays: what reading K members' logits costs when every member also
          writes a mask and an overlay; HIP events around the K calls, the median of --reps.

Prints one JSON line, with the device's clock and power as rocm-smi reports them right after the timed launches."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12                                                # bytes / s, the MI355X's specified peak
THRESHOLD = 0.4


def device_state():
    """Clock and power as rocm-smi reports them (read only); what could not be read is said so."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=60)
        card = next(iter(json.loads(r.stdout).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower() or "power" in k.lower()}
    except Exception as e:                                       # the figure is context, not a result
        return {"not_read": repr(e)}


def events(fn, warmup, reps):
    """-> sorted milliseconds of `reps` calls of fn between HIP events, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in evs)


def time_members(args, K):
    from uia_hip import ops
    from src.utils.viz import NativeMaskWriter
    dev = torch.device("cuda:0")
    B, S, H, W = args.batch, 224, 480, 640
    g = torch.Generator().manual_seed(K)
    flips = [k % 4 for k in range(K)]
    logits = (3 * torch.randn(K, B, 2, S, S, generator=g)).to(dev)
    src = torch.randint(0, 256, (B * H * W,), dtype=torch.uint8, generator=g).to(dev)
    where, total = NativeMaskWriter.layout([(H, W)] * B, overlay=True, prob=True, spread=True)
    desc = torch.tensor([[b * H * W, H, W, moff, ooff, poff, roff, 0] for b, (moff, ooff, poff, roff) in enumerate(where)], dtype=torch.int32).pin_memory()
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    stats, sums = torch.empty(B, 8, dtype=torch.int32, device=dev), torch.empty(B, 2, dtype=torch.int64, device=dev)
    ms = events(lambda: ops.seg_predict_native_ens(logits, flips, src, desc, out, THRESHOLD, stats, sums), args.warmup, args.reps)
    state = device_state()
    moved = logits.numel() * 4 + src.numel() + total

    plain_where, plain_total = NativeMaskWriter.layout([(H, W)] * B, overlay=True)
    plain_desc = torch.tensor([[b * H * W, H, W, moff, ooff, 0, 0, 0] for b, (moff, ooff) in enumerate(plain_where)], dtype=torch.int32).pin_memory()
    plain_out = torch.empty(plain_total, dtype=torch.uint8, device=dev)

    def floor():
        for k in range(K):
            ops.seg_predict_native(logits[k], src, plain_desc, plain_out, stats)
    floor_ms = events(floor, args.warmup, args.reps)

    def eager():
        res = []
        for b in range(B):
            p = []
            for k, f in enumerate(flips):
                planes = logits[k, b:b + 1]
                dims = [d for d, bit in ((-1, 1), (-2, 2)) if f & bit]
                up = F.interpolate(torch.flip(planes, dims) if dims else planes, size=(H, W), mode="bilinear", align_corners=False)[0]
                p.append(torch.sigmoid(up[1] - up[0]))
            p = torch.stack(p)
            P = p.mean(dim=0)
            mask = (P > THRESHOLD).to(torch.uint8) * 255
            gray = src[b * H * W:(b + 1) * H * W].view(H, W)
            res.append((mask, torch.stack([gray, torch.maximum(gray, mask), gray], dim=-1), (255 * P + 0.5).to(torch.uint8),
                        (255 * (p.max(dim=0).values - p.min(dim=0).values) + 0.5).to(torch.uint8)))
        torch.cuda.synchronize()
        return res
    eager()
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eager()
        host.append((time.perf_counter() - t0) * 1e3)
    ops.seg_predict_native_ens(logits, flips, src, desc, out, THRESHOLD, stats, sums)
    flat = out.cpu()
    differ = {"mask": 0, "prob_more_than_1": 0, "spread_more_than_1": 0}
    for (moff, _, poff, roff), (mask, _, q, r) in zip(where, res):
        differ["mask"] += int((flat[moff:moff + H * W].view(H, W) != mask.cpu()).sum())
        differ["prob_more_than_1"] += int(((flat[poff:poff + H * W].view(H, W).int() - q.cpu().int()).abs() > 1).sum())
        differ["spread_more_than_1"] += int(((flat[roff:roff + H * W].view(H, W).int() - r.cpu().int()).abs() > 1).sum())
    med = statistics.median(ms)
    return {"K": K, "launch_ms": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4), "moved_mb": round(moved / 1e6, 2),
            "share_of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4), "eager_loop_ms": round(statistics.median(host), 2),
            "k_plain_launches_ms": round(statistics.median(floor_ms), 4), "pixels_differing_from_torch_fp32": differ, "of": B * H * W, "device": state}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--members", type=int, nargs="+", default=[1, 4, 12])
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_seg_native_ens.py measures on the MI355X: no GPU here, nothing measured")
    print(json.dumps({"batch": args.batch, "S": 224, "H": 480, "W": 640, "reps": args.reps, "threshold": THRESHOLD,
                      "members": [time_members(args, K) for K in args.members]}))


if __name__ == "__main__":
    main()
