"""Float64 restatement of the segmentation surface-distance metrics (MONAI 1.5.1 compute_hausdorff_distance(percentile=...) and
compute_average_surface_distance as the reference's MetricAccumulator calls them, src/utils/tools.py:185-206): binary masks, include_background=False,
spacing=None, Euclidean distance, symmetric HD, directed ASD (prediction -> ground truth).  CPU torch only: no scipy, no oracle.

Per image b:
  1. P = argmax(logits[b]) == 1 (torch's argmax: a tie goes to class 0, NaN is the maximum), G = label[b, 0] > 0;
  2. E(M) = M & ~erode(M), 4-neighbour erosion with out-of-image pixels as background;
  3. d(A->B)[i] = exact Euclidean distance from pixel i of E(A) to the nearest pixel of E(B): integer squared distances by brute force, sqrt in
     float64, cast to float32 (scipy's distance_transform_edt and MONAI's cast);
  4. hd = max(q(d(P->G)), q(d(G->P))), q = torch.quantile(d, percentile / 100) on the float32 distances, except that percentile 0 (falsy) takes the
     maximum, as MONAI's `if not percentile: return surface_distance.max()` does;
  5. asd = mean of d(P->G) (float64 sum of the float32 distances);
  6. an empty P or G: both NaN (the reference's value there is NaN or inf, and its compute() drops it).
"""
import numpy as np
import torch


def masks(logits, label):
    """[B,2,H,W], [B,1,H,W] -> P, G bool [B,H,W] (the masks of src/losses/dice.py::dice_per_image)."""
    return logits.argmax(dim=1) == 1, label[:, 0] > 0


def edges(m):
    """bool [H,W] -> E(m): pixels of m with a 4-neighbour outside m (out of the image counts as outside)."""
    p = torch.nn.functional.pad(m, (1, 1, 1, 1), value=False)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def _offsets(r2max):
    """every (dy, dx) with dy² + dx² <= r2max, grouped by squared length in increasing order."""
    r = int(r2max ** 0.5)
    dy, dx = torch.meshgrid(torch.arange(-r, r + 1), torch.arange(-r, r + 1), indexing="ij")
    s = (dy * dy + dx * dx).flatten()
    off = torch.stack([dy.flatten(), dx.flatten()], 1)
    return [(int(v), off[s == v]) for v in s.unique().tolist() if v <= r2max]


def directed_sq(ea, eb, near=64, chunk=1 << 22):
    """int64 squared distances from every pixel of ea to the nearest pixel of eb (row-major order of ea's pixels).  Exact in two steps: every offset of
    squared length <= `near`, in increasing length (the first hit is the minimum), then brute force in chunks over all of eb for the pixels still open."""
    a = ea.nonzero().to(torch.int64)
    b = eb.nonzero().to(torch.int64)
    H, W = eb.shape
    out = torch.full((a.shape[0],), -1, dtype=torch.int64)
    for s, off in _offsets(near):
        open_ = (out < 0).nonzero()[:, 0]
        if open_.numel() == 0:
            break
        p = a[open_, None, :] + off[None]
        ok = (p[..., 0] >= 0) & (p[..., 0] < H) & (p[..., 1] >= 0) & (p[..., 1] < W)
        hit = torch.zeros(ok.shape, dtype=torch.bool)
        hit[ok] = eb[p[..., 0][ok], p[..., 1][ok]]
        out[open_[hit.any(1)]] = s
    rest = (out < 0).nonzero()[:, 0]
    step = max(1, chunk // max(1, b.shape[0]))
    for i in range(0, rest.numel(), step):
        idx = rest[i:i + step]
        d = a[idx, None, :] - b[None, :, :]
        out[idx] = (d * d).sum(-1).min(1).values
    return out


def distances(sq):
    """integer squared distances -> float32 distances (sqrt in float64, then the cast)."""
    return torch.sqrt(sq.to(torch.float64)).to(torch.float32)


def quantile(d, percentile):
    if not percentile:
        return float(d.max())
    return float(torch.quantile(d, percentile / 100))


def surface_distances(logits, label, percentile=95.0):
    """-> (hd, asd) float64 numpy arrays [B]."""
    logits, label = logits.detach().cpu(), label.detach().cpu()
    P, G = masks(logits, label)
    B = P.shape[0]
    hd, asd = np.full(B, np.nan), np.full(B, np.nan)
    for b in range(B):
        ep, eg = edges(P[b]), edges(G[b])
        if not ep.any() or not eg.any():
            continue
        d_pg = distances(directed_sq(ep, eg))
        d_gp = distances(directed_sq(eg, ep))
        hd[b] = max(quantile(d_pg, percentile), quantile(d_gp, percentile))
        asd[b] = float(d_pg.double().mean())
    return hd, asd


def finite_stats(values):
    """np.mean / np.std (population) over the finite entries: what MetricAccumulator.compute() reports; NaN when none is finite."""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return (float(np.mean(v)), float(np.std(v))) if v.size else (float("nan"), float("nan"))
