"""Top-K listing: the fused kernel (uia_retrieval_topk, csrc/retrieval.hip) against the eager PyTorch form and against the rank-count call it shares
its score tiles with, on the same device and data (reported in DESIGN.md §4 "Retrieval").

  fused:  ops.retrieval_topk(img, txt, 10)                     (one direction; idx and score [n, 10]; the n x n matrix is never written)
  eager:  an, bn = F.normalize(img), F.normalize(txt);  torch.topk(an @ bn.T, 10)          (the n x n matrix)
  ranks:  ops.retrieval_ranks(img, txt)                        (both directions' counts from the same score FLOPs as ONE direction of the listing)

at E = 512, K = 10 for every paired n of --sizes (default 10000, the ROCOv2 test split, and 60000, its train split), and one free query against the
largest gallery (the column-split path).  Per n and form: the median of HIP-event times over --reps calls (a third of them, at least 3, above 20000)
after --warmup calls; for the fused and the eager form torch.cuda.max_memory_allocated over those calls less the bytes of the two inputs.  The two
forms' index lists are compared: eager orders its sums differently and breaks ties its own way, so rows may differ; their number is reported, not
asserted.  Prints one JSON line."""
import argparse
import json
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


def measure(fn, warmup, reps, base):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    ms = timed(fn, warmup, reps)
    return ms, round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def eager_topk(q, g, k):
    an, bn = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(g, dim=-1)
    return torch.topk(an @ bn.T, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 60000])
    args = ap.parse_args()
    from uia_hip import _lib, ops
    dev = torch.device("cuda:0")
    K = args.k
    out = {"embed": args.embed, "k": K}
    for N in args.sizes:
        g = torch.Generator().manual_seed(N)
        img = torch.randn(N, args.embed, generator=g)
        txt = (img + 3.0 * torch.randn(N, args.embed, generator=g)).to(dev)
        img = img.to(dev)
        base = torch.cuda.memory_allocated()
        reps = args.reps if N <= 20000 else max(3, args.reps // 3)
        f_ms, f_mib = measure(lambda: ops.retrieval_topk(img, txt, K), args.warmup, reps, base)
        r_ms, _ = measure(lambda: ops.retrieval_ranks(img, txt), args.warmup, reps, base)
        e_ms, e_mib = measure(lambda: eager_topk(img, txt, K), min(args.warmup, 2), reps, base)
        fused_idx = ops.retrieval_topk(img, txt, K)[0].long()
        eager_idx = eager_topk(img, txt, K).indices
        rows = int((fused_idx != eager_idx).any(1).sum())
        del eager_idx, fused_idx
        out[f"n{N}"] = {"fused_ms": f_ms, "fused_peak_mib": f_mib, "workspace_mib": round(_lib.lib().uia_retrieval_topk_workspace_bytes(N, N, args.embed, K) / 2 ** 20, 1),
                        "eager_ms": e_ms, "eager_peak_mib": e_mib, "ranks_ms": r_ms, "fused_over_ranks": round(f_ms / r_ms, 2),
                        "eager_over_fused": round(e_ms / f_ms, 2), "rows_with_differing_lists": rows}
        if N == max(args.sizes):                                  # one free query: the grid is the column splits alone
            one = img[:1].contiguous()
            s_ms, _ = measure(lambda: ops.retrieval_topk(one, txt, K), args.warmup, args.reps, base)
            u_ms, _ = measure(lambda: ops.retrieval_topk(one, txt, K, splits=1), args.warmup, args.reps, base)
            o_ms, _ = measure(lambda: eager_topk(one, txt, K), args.warmup, args.reps, base)
            out[f"q1_n{N}"] = {"fused_ms": s_ms, "splits": _lib.lib().uia_retrieval_topk_splits(1, N), "fused_one_split_ms": u_ms, "eager_ms": o_ms}
        del img, txt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
