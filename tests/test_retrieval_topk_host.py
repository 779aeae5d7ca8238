"""Host checks of the top-K listing: the float64 restatement (tests/retrieval_topk_reference.py) against a brute-force sort; the argument checks of
uia_retrieval_topk, which fail before any launch; the workspace formula and the column-split rule; write_topk_csv; the entry point's two flags."""
import csv
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import retrieval_topk_reference as T  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restatement
def _before(a, b):
    """(score, index) a comes before b: the order of the listing, written out case by case."""
    (s, i), (t, j) = a, b
    if math.isnan(s) or math.isnan(t):
        if math.isnan(s) != math.isnan(t):
            return math.isnan(t)
        return i < j
    if s != t:                                                   # IEEE: +0 == -0
        return s > t
    return i < j


def test_restatement_equals_a_brute_force_sort_with_ties_nan_and_signed_zeros():
    rng = np.random.default_rng(5)
    S = rng.integers(-2, 3, (7, 9)).astype(np.float64)           # five values over nine columns: ties in every row
    S[1, 4] = np.nan
    S[2, :] = np.nan                                             # a NaN query row: 0 .. K-1
    S[3, 2], S[3, 6], S[3, 7] = 0.0, -0.0, 0.0
    S[4, :] = -1.0
    S[4, 3], S[4, 5] = -0.0, 0.0                                 # -0 at the lower index must come first: the zeros are equal
    S[5, 0], S[5, 8] = -np.inf, np.nan                           # -inf stays above NaN
    S[6, 1] = np.inf
    for K in (1, 4, 9):
        idx, score = T.topk(S, K)
        assert idx.shape == (7, K) and score.shape == (7, K)
        for q in range(7):
            want = sorted(range(9), key=functools.cmp_to_key(lambda i, j: -1 if _before((S[q, i], i), (S[q, j], j)) else 1))[:K]
            assert idx[q].tolist() == want, (K, q, idx[q].tolist(), want)
            assert np.array_equal(score[q], S[q, want], equal_nan=True)
    idx, _ = T.topk(S, 9)
    assert idx[2].tolist() == list(range(9)) and idx[1, -1] == 4 and idx[5, -2:].tolist() == [0, 8]
    assert idx[4, :2].tolist() == [3, 5] and idx[3].tolist().index(2) < idx[3].tolist().index(6) < idx[3].tolist().index(7)


# ------------------------------------------------------------------------------------------------ the C entries without a GPU
def test_topk_entries_are_declared_exported_and_typed():
    import ctypes
    from uia_hip import _lib
    src = open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uia_retrieval_topk_workspace_bytes", "uia_retrieval_topk_splits", "uia_retrieval_topk"):
        assert name + "(" in src and hasattr(handle, name) and name in _lib.PROTOTYPES, name


def test_topk_argument_checks_fail_before_any_launch():
    from uia_hip import _lib
    lib = _lib.lib()
    need = lib.uia_retrieval_topk_workspace_bytes(300, 200, 64, 10)
    assert need >= (300 + 200) * 64 * 4
    fake = 4096                                                  # never dereferenced: every case below is refused by the argument checks

    def call(Q=300, N=200, E=64, K=10, q=fake, g=fake, normalize=1, splits=0, ws=fake, ws_bytes=need, idx=fake, score=fake):
        return lib.uia_retrieval_topk(None, Q, N, E, K, q, g, normalize, splits, ws, ws_bytes, idx, score)

    for kw, text in ((dict(K=0), b"K="), (dict(K=33), b"K="), (dict(K=-1), b"K="), (dict(N=8, K=9), b"K="), (dict(E=6), b"E="), (dict(E=0), b"E="),
                     (dict(E=4100), b"E="), (dict(Q=0), b"Q="), (dict(N=0), b"N="), (dict(Q=(1 << 24) + 1), b"Q="), (dict(N=(1 << 24) + 1), b"N="),
                     (dict(q=None), b"null"), (dict(g=None), b"null"), (dict(ws=None), b"null"), (dict(idx=None), b"null"), (dict(score=None), b"null"),
                     (dict(q=fake + 4), b"aligned"), (dict(g=fake + 4), b"aligned"), (dict(ws=fake + 8), b"aligned"), (dict(idx=fake + 2), b"aligned"),
                     (dict(splits=-1), b"splits"), (dict(splits=100000), b"splits"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_retrieval_topk" in msg and text in msg, (kw, msg)


def test_topk_workspace_is_zero_outside_the_limits_and_never_grows_with_q_times_n():
    from uia_hip import _lib
    lib = _lib.lib()
    for Q, N, E, K in ((0, 10, 8, 1), (10, 0, 8, 1), (10, 10, 6, 1), (10, 10, 0, 1), (10, 10, 4100, 1), (10, 10, 8, 0), (10, 10, 8, 33), (10, 10, 8, 11),
                       ((1 << 24) + 1, 10, 8, 1), (10, (1 << 24) + 1, 8, 1)):
        assert lib.uia_retrieval_topk_workspace_bytes(Q, N, E, K) == 0, (Q, N, E, K)
    big = lib.uia_retrieval_topk_workspace_bytes(60000, 60000, 512, 10)
    assert 2 * 60000 * 512 * 4 <= big < 1 << 30, big                        # the score matrix alone would be 14.4 GB
    # beyond the two normalised copies: the partial lists, at most 512 x 128 x K entries of 8 bytes whatever N is
    for Q, N, K in ((1, 60000, 10), (1, 1 << 24, 32), (130, 1 << 20, 32), (60000, 60000, 32), (1 << 24, 1 << 24, 32)):
        extra = lib.uia_retrieval_topk_workspace_bytes(Q, N, 4, K) - (Q + N) * 4 * 4
        assert 0 <= extra <= 512 * 128 * K * 8 + 4 * 256, (Q, N, K, extra)


def test_topk_split_rule():
    from uia_hip import _lib
    lib = _lib.lib()
    for Q, N in ((1, 1), (1, 128), (1, 129), (97, 97), (130, 517), (1, 60000), (60000, 60000), (1 << 24, 1 << 24), (1, 1 << 24), (128 * 256 + 1, 60000)):
        s = lib.uia_retrieval_topk_splits(Q, N)
        assert 1 <= s <= (N + 127) // 128, (Q, N, s)                         # never an empty strip
    assert lib.uia_retrieval_topk_splits(128 * 256 + 1, 60000) == 1          # 257 row tiles: more than the 256 CUs
    assert lib.uia_retrieval_topk_splits(60000, 60000) == 1
    assert lib.uia_retrieval_topk_splits(1, 60000) > 1
    assert lib.uia_retrieval_topk_splits(1, 100) == 1 and lib.uia_retrieval_topk_splits(1, 300) == 3


def test_retrieval_topk_ops_refuse_cpu_tensors():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    from src.utils.retrieval_metrics import retrieve_topk
    with pytest.raises(UiaError):
        ops.retrieval_topk(torch.randn(8, 16), torch.randn(9, 16), 3)
    with pytest.raises(UiaError):
        retrieve_topk(torch.randn(8, 16), torch.randn(9, 16), 3)


# ------------------------------------------------------------------------------------------------ the listing as a table
def test_write_topk_csv_round_trips_captions_with_commas_and_quotes(tmp_path):
    from src.utils.retrieval_metrics import write_topk_csv
    captions = ['CT of the chest, axial: "ground glass" opacity', "plain", 'a "quoted", comma\'d one']
    idx = torch.tensor([[0, 2], [2, 1], [1, 0]], dtype=torch.int32)
    score = torch.tensor([[0.5, 0.25], [1.0, -0.125], [0.1234564, float("nan")]])
    header = ["query_index", "rank", "candidate_index", "score", "is_pair", "caption"]
    write_topk_csv(tmp_path / "i2t.csv", idx, score, captions, "i2t")
    rows = list(csv.reader(open(tmp_path / "i2t.csv", newline="")))
    assert rows[0] == header and len(rows) == 7
    assert rows[1] == ["0", "1", "0", "0.500000", "1", captions[0]] and rows[2] == ["0", "2", "2", "0.250000", "0", captions[2]]
    assert rows[3] == ["1", "1", "2", "1.000000", "0", captions[2]] and rows[4] == ["1", "2", "1", "-0.125000", "1", captions[1]]
    assert rows[5] == ["2", "1", "1", "0.123456", "0", captions[1]] and rows[6] == ["2", "2", "0", "nan", "0", captions[0]]
    write_topk_csv(tmp_path / "t2i.csv", idx, score, captions, "t2i")
    rows = list(csv.reader(open(tmp_path / "t2i.csv", newline="")))
    assert [r[5] for r in rows[1:]] == [captions[0], captions[0], captions[1], captions[1], captions[2], captions[2]]       # the query's caption
    assert [r[4] for r in rows[1:]] == ["1", "0", "0", "1", "0", "0"]
    write_topk_csv(tmp_path / "q.csv", idx[:2], score[:2], ['first, "query"', "second"], "queries")
    rows = list(csv.reader(open(tmp_path / "q.csv", newline="")))
    assert [r[5] for r in rows[1:]] == ['first, "query"', 'first, "query"', "second", "second"] and all(r[4] == "0" for r in rows[1:])


def test_hit_at_k_counts_own_pairs_inside_the_first_k():
    from src.utils.retrieval_metrics import hit_at_k
    idx = torch.tensor([[0, 3, 2], [2, 1, 0], [0, 1, 3], [1, 2, 3]], dtype=torch.int32)
    assert hit_at_k(idx, [1, 2, 3, 5]) == {1: 25.0, 2: 50.0, 3: 75.0}


# ------------------------------------------------------------------------------------------------ command line
def test_get_args_topk_defaults_and_refusals(capsys):
    from src.models.biomedclip import retrieval
    a = retrieval.get_args([])
    assert a.topk == 0 and a.queries_txt is None
    b = retrieval.get_args(["--topk", "32", "--queries_txt", "q.txt"])
    assert b.topk == 32 and b.queries_txt == "q.txt"
    for argv in (["--queries_txt", "q.txt"], ["--topk", "33"], ["--topk", "-1"], ["--topk", "0", "--queries_txt", "q.txt"]):
        with pytest.raises(SystemExit):
            retrieval.get_args(argv)
    assert "--topk" in capsys.readouterr().err
