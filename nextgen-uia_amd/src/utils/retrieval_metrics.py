"""Image-text retrieval metrics — the module the reference's retrieval entry point imports (src/models/biomedclip/retrieval.py:15) and calls (:329, :332)
but never shipped.  The call signatures and the keys the entry point reads (:233-248) are the reference's; the definitions are this build's:

  * scores s_ij = <image feature i, text feature j> in fp32 (L2-normalised rows when `normalize`); pair i belongs together;
  * ranks are OPTIMISTIC: rank = 1 + #{others scoring strictly above the query's own pair}, the usual `(sim > sim.diag()[:, None]).sum(1)` form, so a tie
    never costs a place.  `i2t_ties` / `t2i_ties` count the queries with at least one other candidate scoring exactly what their own pair scores;
  * `{d}_r@{k}` = 100 · #{rank <= k} / n, `{d}_medr` the median rank (numpy.median), `{d}_meanr` the mean rank, for d = i2t (an image queries the texts)
    and t2i; `rsum` is the sum of every R@K of both directions.

Everything up to the record runs on the device: `uia_retrieval_ranks` forms score tiles on the fp32 matrix cores and reduces them to rank counts without
writing the n x n matrix, `uia_retrieval_stats` turns one direction's counts into R@K / median / mean.  One host copy brings both records and the tie counts.

The listing behind the table is `retrieve_topk` (`uia_retrieval_topk`: the same score tiles with a selection epilogue): each query's K best candidates,
score descending, EQUAL scores by candidate index ascending, NaN scores last.  That tie rule is by index where the metrics' is optimistic, so the share of
queries whose own pair is in their K-list (`hit_at_k`) is at most R@K; the gap is what ties are worth.  `write_topk_csv` writes a listing as a table."""
import csv
import logging

import torch


def assemble_metrics(host, k_values):
    """host: the flat list [i2t record (len(k) + 2), t2i record (len(k) + 2), i2t ties, t2i ties, n] -> the metrics dict of Python floats."""
    nk = len(k_values)
    assert len(host) == 2 * (nk + 2) + 3, (len(host), nk)
    out = {}
    for d, rec in (("i2t", host[:nk + 2]), ("t2i", host[nk + 2:2 * (nk + 2)])):
        for k, v in zip(k_values, rec):
            out[f"{d}_r@{k}"] = float(v)
        out[f"{d}_medr"] = float(rec[nk])
        out[f"{d}_meanr"] = float(rec[nk + 1])
    out["rsum"] = float(sum(out[f"{d}_r@{k}"] for d in ("i2t", "t2i") for k in k_values))
    out["i2t_ties"], out["t2i_ties"], out["n"] = float(host[-3]), float(host[-2]), float(host[-1])
    return out


def compute_retrieval_metrics(image_features, text_features, k_values=(1, 5, 10), normalize=True):
    """image_features, text_features: device tensors [n, D], row i of one paired with row i of the other -> dict of Python floats (keys above)."""
    from uia_hip import ops
    k_values = [int(k) for k in k_values]
    gt_i2t, eq_i2t, gt_t2i, eq_t2i = ops.retrieval_ranks(image_features, text_features, normalize=normalize)
    rec_i = ops.retrieval_stats(gt_i2t, k_values)
    rec_t = ops.retrieval_stats(gt_t2i, k_values)
    ties = torch.stack([(eq_i2t > 0).sum(), (eq_t2i > 0).sum()]).double()
    host = torch.cat([rec_i, rec_t, ties]).cpu().tolist()          # one device-to-host copy
    return assemble_metrics(host + [gt_i2t.numel()], k_values)


def log_retrieval_metrics(metrics, prefix=""):
    """One line per direction and the summary, on the root logger."""
    ks = sorted(int(k[len("i2t_r@"):]) for k in metrics if k.startswith("i2t_r@"))
    tag = f"[{prefix}] " if prefix else ""
    for d, name in (("i2t", "Image-to-Text"), ("t2i", "Text-to-Image")):
        rk = "  ".join(f"R@{k}: {metrics[f'{d}_r@{k}']:.2f}" for k in ks)
        logging.info(f"{tag}{name}: {rk}  MedR: {metrics[f'{d}_medr']:.1f}  MeanR: {metrics[f'{d}_meanr']:.1f}")
    extra = ""
    if "n" in metrics:
        extra = f"  (n={int(metrics['n'])}, queries with ties: i2t {int(metrics.get('i2t_ties', 0))}, t2i {int(metrics.get('t2i_ties', 0))})"
    logging.info(f"{tag}rSum: {metrics['rsum']:.2f}{extra}")


def retrieve_topk(query_features, gallery_features, k, normalize=True):
    """query_features [Q, D], gallery_features [N, D] device tensors, 1 <= k <= min(N, 32) -> (idx int32 [Q, k], score fp32 [Q, k]) device tensors:
    idx[q, r] is the gallery row at place r + 1 for query q (order above), score[q, r] its score.  The Q x N matrix is never formed."""
    from uia_hip import ops
    return ops.retrieval_topk(query_features, gallery_features, int(k), normalize=normalize)


def hit_at_k(idx, k_values):
    """idx [n, K] of a PAIRED listing (query i belongs to candidate i) -> {k: percent of queries whose own pair is among their first k} for each k <= K."""
    n, K = idx.shape
    own = idx == torch.arange(n, device=idx.device, dtype=idx.dtype)[:, None]
    return {int(k): 100.0 * float(own[:, :int(k)].any(1).sum()) / n for k in k_values if int(k) <= K}


TOPK_COLUMNS = ("query_index", "rank", "candidate_index", "score", "is_pair", "caption")


def write_topk_csv(path, idx, score, captions, direction):
    """One row per (query, place): query_index, rank (1-based), candidate_index, score (%.6f), is_pair (candidate_index == query_index) and the text side of
    the row: the candidate's caption for direction "i2t", the query's caption for "t2i".  Direction "queries" is free-text queries against the images:
    `captions` are the query lines, caption is the query's and is_pair is always 0."""
    assert direction in ("i2t", "t2i", "queries"), direction
    idx, score = torch.as_tensor(idx).cpu().tolist(), torch.as_tensor(score).cpu().tolist()
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(TOPK_COLUMNS)
        for q, (row_i, row_s) in enumerate(zip(idx, score)):
            for r, (c, s) in enumerate(zip(row_i, row_s)):
                pair = int(c == q) if direction != "queries" else 0
                w.writerow([q, r + 1, c, f"{s:.6f}", pair, captions[c] if direction == "i2t" else captions[q]])
