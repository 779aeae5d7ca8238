"""Retrieval rank counts: the fused kernel (uia_retrieval_ranks, csrc/retrieval.hip) against the eager PyTorch formulation on the same device and data
(reported in DESIGN.md §4).

  eager:  a, b = F.normalize(img), F.normalize(txt);  S = a @ b.T;  d = S.diag()
          gt_i2t = (S > d[:, None]).sum(1);  gt_t2i = (S > d[None, :]).sum(0)           (the N x N matrix and a boolean temporary of its extent)
  fused:  ops.retrieval_ranks(img, txt)                                                 (four count vectors; the matrix is never written)

at E = 512 for every N of --sizes (default 10000, the ROCOv2 test split, and 60000, its train split) and, with --largest, at the largest N (a multiple
of 1000, at most --max_n) whose eager form fits into 80 % of the device memory that is free when the tool starts, counting 13 bytes per score (S, the
boolean, and the int64 copy of it that torch's sum makes: the measured peak).
Per N and form: the median of HIP-event times over --reps calls after --warmup calls, and torch.cuda.max_memory_allocated over those calls less the
bytes of the two inputs.  The two forms' counts are compared (eager orders its sums differently, so a few near-ties may differ; the number of queries
that differ is reported, not asserted).  Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]
import torch  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def eager_ranks(img, txt):
    a, b = torch.nn.functional.normalize(img, dim=-1), torch.nn.functional.normalize(txt, dim=-1)
    S = a @ b.T
    d = S.diag()
    return (S > d[:, None]).sum(1), (S > d[None, :]).sum(0)


def measure(fn, warmup, reps, base):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(fn, warmup, reps)
    return ms, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 60000])
    ap.add_argument("--largest", action="store_true", help="also run at the largest N whose eager form fits into 80 %% of the free device memory")
    ap.add_argument("--max_n", type=int, default=120000)
    args = ap.parse_args()
    from uia_hip import ops
    dev = torch.device("cuda:0")
    sizes = list(args.sizes)
    if args.largest:
        free, _ = torch.cuda.mem_get_info(dev)
        n = int(math.sqrt(0.8 * free / 13.0)) // 1000 * 1000
        sizes.append(max(1000, min(n, args.max_n)))
    out = {"embed": args.embed}
    for N in sizes:
        g = torch.Generator().manual_seed(N)
        img = torch.randn(N, args.embed, generator=g)
        txt = (img + 3.0 * torch.randn(N, args.embed, generator=g)).to(dev)
        img = img.to(dev)
        base = torch.cuda.memory_allocated()
        reps = args.reps if N <= 20000 else max(3, args.reps // 3)
        f_ms, f_mib = measure(lambda: ops.retrieval_ranks(img, txt), args.warmup, reps, base)
        e_ms, e_mib = measure(lambda: eager_ranks(img, txt), min(args.warmup, 2), reps, base)
        fused = ops.retrieval_ranks(img, txt)
        eager = eager_ranks(img, txt)
        diff = [int((fused[0].long() != eager[0]).sum()), int((fused[2].long() != eager[1]).sum())]
        del eager, fused, img, txt
        out[f"n{N}"] = {"fused_ms": f_ms, "fused_peak_mib": f_mib, "eager_ms": e_ms, "eager_peak_mib": e_mib, "speedup": round(e_ms / f_ms, 2),
                        "queries_differing_i2t_t2i": diff}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
