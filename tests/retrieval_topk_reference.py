"""Float64 numpy restatement of the top-K listing (uia_retrieval_topk, csrc/retrieval.hip).  A plain module, no pytest.

  topk(S, K)        (idx int64 [Q, K], score float64 [Q, K]): row q holds the first K columns of S[q] under ONE total order: score descending by IEEE
                    comparison (+0 == -0), equal scores by column index ascending; a NaN score below every non-NaN score, NaN scores among themselves
                    by index ascending.  score[q, r] = S[q, idx[q, r]] (NaN where the score is NaN).
Scores come from retrieval_reference.scores."""
import numpy as np


def topk(S, K):
    S = np.asarray(S, dtype=np.float64)
    Q, N = S.shape
    assert 1 <= K <= N
    nan = np.isnan(S)
    key = np.where(nan, -np.inf, S) + 0.0            # -0 + 0 = +0: one key for both zeros; a true -inf is told from NaN by the middle key below
    cols = np.broadcast_to(np.arange(N), (Q, N))
    idx = np.empty((Q, K), dtype=np.int64)
    for q in range(Q):
        order = np.lexsort((cols[q], nan[q], -key[q]))          # last key first: -score, then NaN after non-NaN, then index
        idx[q] = order[:K]
    return idx, np.take_along_axis(S, idx, axis=1)
