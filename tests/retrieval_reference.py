"""Float64 numpy restatement of the retrieval evaluation (csrc/retrieval.hip, src/utils/retrieval_metrics.py).  A plain module, no pytest.

  scores(img, txt, normalize)        s_ij = <a_i, b_j> in float64; a, b the rows divided by max(||row||, 1e-12) when normalize
  counts(S, margin=0)                (gt_i2t, eq_i2t, gt_t2i, eq_t2i), int64: for row i the j != i with S_ij > d_i + margin (gt) and, margin 0 only,
                                     S_ij == d_i (eq); for column j the i != j against d_j.  A query whose d is not finite: gt = N - 1, eq = 0
  stats(gt, k_values)                [R@K ..., median rank, mean rank] of rank = 1 + gt
  metrics(S or counts, k_values)     the dict of compute_retrieval_metrics
Ranks are optimistic (rank = 1 + strictly-greater count); rsum is the sum of every R@K of both directions."""
import numpy as np


def scores(img, txt, normalize=True):
    a, b = np.asarray(img, dtype=np.float64), np.asarray(txt, dtype=np.float64)
    if normalize:
        a = a / np.maximum(np.sqrt((a * a).sum(1, keepdims=True)), 1e-12)
        b = b / np.maximum(np.sqrt((b * b).sum(1, keepdims=True)), 1e-12)
    with np.errstate(invalid="ignore"):
        return a @ b.T


def counts(S, margin=0.0):
    S = np.asarray(S, dtype=np.float64)
    N = S.shape[0]
    assert S.shape == (N, N)
    d = np.diag(S).copy()
    off = ~np.eye(N, dtype=bool)
    bad = ~np.isfinite(d)
    with np.errstate(invalid="ignore"):
        gt_r = ((S > (d + margin)[:, None]) & off).sum(1)
        eq_r = ((S == d[:, None]) & off).sum(1)
        gt_c = ((S > (d + margin)[None, :]) & off).sum(0)
        eq_c = ((S == d[None, :]) & off).sum(0)
    gt_r[bad], gt_c[bad], eq_r[bad], eq_c[bad] = N - 1, N - 1, 0, 0
    return gt_r.astype(np.int64), eq_r.astype(np.int64), gt_c.astype(np.int64), eq_c.astype(np.int64)


def stats(gt, k_values):
    rank = np.asarray(gt, dtype=np.int64) + 1
    n = len(rank)
    return [100.0 * float((rank <= k).sum()) / n for k in k_values] + [float(np.median(rank)), float(np.mean(rank.astype(np.float64)))]


def metrics(S_or_counts, k_values):
    gt_r, eq_r, gt_c, eq_c = S_or_counts if isinstance(S_or_counts, tuple) else counts(S_or_counts)
    out = {}
    for d, gt in (("i2t", gt_r), ("t2i", gt_c)):
        rec = stats(gt, k_values)
        for k, v in zip(k_values, rec):
            out[f"{d}_r@{k}"] = v
        out[f"{d}_medr"], out[f"{d}_meanr"] = rec[-2], rec[-1]
    out["rsum"] = float(sum(out[f"{d}_r@{k}"] for d in ("i2t", "t2i") for k in k_values))
    out["i2t_ties"], out["t2i_ties"], out["n"] = float((eq_r > 0).sum()), float((eq_c > 0).sum()), float(len(gt_r))
    return out
