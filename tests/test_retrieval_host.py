"""Host checks of the retrieval evaluation: the float64 restatement (tests/retrieval_reference.py) and the host-side assembly of
compute_retrieval_metrics against values worked out by hand; the C entries' argument checks, which fail before any launch; the entry point's command
line against the reference's argparse table (tests/golden/reference_cli_retrieval.json, written by tools/gen_retrieval_cli_table.py); the data module."""
import ast
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import retrieval_reference as R  # noqa: E402

# One tie (S[0][2] equals d_0) and one negative diagonal (d_1): rows are images, columns texts.
S4 = np.array([[0.9, 0.1, 0.9, 0.2],
               [0.5, -0.3, 0.0, -0.5],
               [0.3, 0.2, 0.4, 0.6],
               [0.1, 0.7, 0.2, 0.8]])


# ------------------------------------------------------------------------------------------------ hand-checked values
def test_counts_of_the_four_by_four_case():
    gt_r, eq_r, gt_c, eq_c = R.counts(S4)
    assert gt_r.tolist() == [0, 2, 1, 0]            # row 1: 0.5 and 0.0 beat -0.3; row 2: 0.6 beats 0.4; the tie in row 0 costs no place
    assert eq_r.tolist() == [1, 0, 0, 0]
    assert gt_c.tolist() == [0, 3, 1, 0]            # column 1: 0.1, 0.2, 0.7 beat -0.3; column 2: 0.9 beats 0.4
    assert eq_c.tolist() == [0, 0, 0, 0]


def test_metrics_of_the_four_by_four_case():
    m = R.metrics(S4, (1, 2))
    # i2t ranks 1, 3, 2, 1; t2i ranks 1, 4, 2, 1
    want = {"i2t_r@1": 50.0, "i2t_r@2": 75.0, "i2t_medr": 1.5, "i2t_meanr": 1.75, "t2i_r@1": 50.0, "t2i_r@2": 75.0, "t2i_medr": 1.5, "t2i_meanr": 2.0,
            "rsum": 250.0, "i2t_ties": 1.0, "t2i_ties": 0.0, "n": 4.0}
    assert m == want


def test_margin_and_non_finite_diagonal():
    lo = R.counts(S4, margin=0.15)
    hi = R.counts(S4, margin=-0.15)
    assert lo[0].tolist() == [0, 2, 1, 0] and hi[0].tolist() == [1, 2, 2, 1]          # d_0 - 0.15 lets the tie count; 0.3 > 0.25; 0.7 > 0.65
    assert lo[2].tolist() == [0, 3, 1, 0] and hi[2].tolist() == [0, 3, 1, 0]
    bad = S4.copy()
    bad[1, :] = np.nan                                                                  # image 1 is NaN: its row, and the diagonal of column 1
    gt_r, eq_r, gt_c, eq_c = R.counts(bad)
    assert gt_r.tolist() == [0, 3, 1, 0] and gt_c.tolist() == [0, 3, 1, 0]            # worst rank for query 1 in both directions, counted nowhere else
    assert eq_r.tolist() == [1, 0, 0, 0] and eq_c.tolist() == [0, 0, 0, 0]


def test_scores_normalise_rows_with_the_eps_of_f_normalize():
    img = np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    txt = np.array([[6.0, 8.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0]])
    assert R.scores(img, txt, normalize=False).tolist() == [[50.0, 8.0], [0.0, 0.0]]
    S = R.scores(img, txt, normalize=True)
    assert np.allclose(S, [[1.0, 0.8], [0.0, 0.0]], atol=1e-15) and not np.isnan(S).any()         # the zero row stays zero: 0 / 1e-12


def test_stats_median_and_k_above_n():
    assert R.stats([0], (1,)) == [100.0, 1.0, 1.0]
    assert R.stats([4, 0], (1, 2, 5, 10)) == [50.0, 50.0, 100.0, 100.0, 3.0, 3.0]
    assert R.stats([6, 0, 2, 2, 1, 0, 3], (1, 2)) == [100.0 * 2 / 7, 100.0 * 3 / 7, 3.0, 3.0]


def test_assemble_metrics_orders_the_two_records():
    from src.utils.retrieval_metrics import assemble_metrics
    host = [50.0, 75.0, 1.5, 1.75, 25.0, 100.0, 2.0, 2.25, 1.0, 0.0, 4]
    m = assemble_metrics(host, [1, 2])
    assert m == {"i2t_r@1": 50.0, "i2t_r@2": 75.0, "i2t_medr": 1.5, "i2t_meanr": 1.75, "t2i_r@1": 25.0, "t2i_r@2": 100.0, "t2i_medr": 2.0,
                 "t2i_meanr": 2.25, "rsum": 250.0, "i2t_ties": 1.0, "t2i_ties": 0.0, "n": 4.0}
    assert all(type(v) is float for v in m.values())
    with pytest.raises(AssertionError):
        assemble_metrics(host[:-1], [1, 2])


def test_log_retrieval_metrics_writes_both_directions(caplog):
    import logging
    from src.utils.retrieval_metrics import log_retrieval_metrics
    with caplog.at_level(logging.INFO):
        log_retrieval_metrics(R.metrics(S4, (1, 2)), prefix="test")
    text = caplog.text
    assert "[test] Image-to-Text: R@1: 50.00  R@2: 75.00  MedR: 1.5  MeanR: 1.8" in text and "Text-to-Image" in text and "rSum: 250.00" in text


# ------------------------------------------------------------------------------------------------ the C entries without a GPU
def test_retrieval_entries_are_declared_exported_and_typed():
    import ctypes
    from uia_hip import _lib
    src = open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uia_retrieval_workspace_bytes", "uia_retrieval_ranks", "uia_retrieval_stats_workspace_bytes", "uia_retrieval_stats"):
        assert name + "(" in src and hasattr(handle, name) and name in _lib.PROTOTYPES, name


def test_retrieval_ranks_argument_checks_fail_before_any_launch():
    from uia_hip import _lib
    lib = _lib.lib()
    need = lib.uia_retrieval_workspace_bytes(300, 64)
    assert need >= 300 * 4 + 2 * 300 * 64 * 4
    for N, E in ((0, 64), (300, 6), (300, 4100), (300, 0), ((1 << 24) + 1, 64)):
        assert lib.uia_retrieval_workspace_bytes(N, E) == 0, (N, E)
    fake = 4096                                                  # never dereferenced: every case below is refused by the argument checks

    def call(N=300, E=64, img=fake, txt=fake, normalize=1, ws=fake, ws_bytes=need, a=fake, b=fake, c=fake, d=fake):
        return lib.uia_retrieval_ranks(None, N, E, img, txt, normalize, ws, ws_bytes, a, b, c, d)

    for kw, text in ((dict(img=None), b"null"), (dict(txt=None), b"null"), (dict(ws=None), b"null"), (dict(a=None), b"null"), (dict(b=None), b"null"),
                     (dict(c=None), b"null"), (dict(d=None), b"null"), (dict(N=0), b"bad shape"), (dict(N=-1), b"bad shape"),
                     (dict(N=(1 << 24) + 1), b"bad shape"), (dict(E=6), b"bad shape"), (dict(E=4100), b"bad shape"), (dict(E=0), b"bad shape"),
                     (dict(img=fake + 4), b"aligned"), (dict(ws_bytes=need - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_retrieval_ranks" in msg and text in msg, (kw, msg)


def test_retrieval_stats_argument_checks_fail_before_any_launch():
    import ctypes
    from uia_hip import _lib
    lib = _lib.lib()
    need = lib.uia_retrieval_stats_workspace_bytes(100)
    assert need > 0 and lib.uia_retrieval_stats_workspace_bytes(0) == 0
    fake = 4096

    def ks(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def call(N=100, gt=fake, nk=2, k=ks(1, 5), ws=fake, ws_bytes=need, rec=fake):
        return lib.uia_retrieval_stats(None, N, gt, nk, k, ws, ws_bytes, rec)

    for kw, text in ((dict(gt=None), b"null"), (dict(k=None), b"null"), (dict(ws=None), b"null"), (dict(rec=None), b"null"), (dict(N=0), b"bad size"),
                     (dict(nk=0), b"bad count"), (dict(nk=17, k=ks(*range(1, 18))), b"bad count"), (dict(k=ks(1, 0)), b"bad K"), (dict(k=ks(-3, 2)), b"bad K"),
                     (dict(ws_bytes=need - 1), b"workspace")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_retrieval_stats" in msg and text in msg, (kw, msg)


def test_retrieval_ops_refuse_cpu_tensors():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    with pytest.raises(UiaError):
        ops.retrieval_ranks(torch.randn(8, 16), torch.randn(8, 16))
    with pytest.raises(UiaError):
        ops.retrieval_stats(torch.zeros(8, dtype=torch.int32), (1, 5))
    from src.utils.retrieval_metrics import compute_retrieval_metrics
    with pytest.raises(UiaError):
        compute_retrieval_metrics(torch.randn(8, 16), torch.randn(8, 16))


# ------------------------------------------------------------------------------------------------ command line
ADDITIONS = ("--dtype", "--synthetic", "--synthetic_test", "--data_pt", "--ckpt_path", "--model_config")


def test_retrieval_cli_carries_every_reference_flag_and_default():
    from oracle.gen_host_fixtures import argparse_table
    from src.models.biomedclip import retrieval
    ref = json.load(open(os.path.join(HERE, "golden", "reference_cli_retrieval.json")))["biomedclip/retrieval.py"]
    assert len(ref) == 21
    got = argparse_table(os.path.join(ROOT, "nextgen-uia_amd/src/models/biomedclip/retrieval.py"))
    args = vars(retrieval.get_args([]))
    for flag, kw in ref.items():
        assert flag in got, flag
        if flag == "--device":                                   # decided without a HIP call (tools.default_device)
            continue
        assert got[flag] == kw, (flag, kw, got[flag])
        if "default" in kw:
            assert args[flag[2:]] == ast.literal_eval(kw["default"]), flag
    for flag in ADDITIONS:
        assert flag[2:] in args, flag


def test_get_args_defaults_and_parsing():
    from src.models.biomedclip import retrieval
    a = retrieval.get_args([])
    assert a.k_values == [1, 2, 5, 10] and a.split == "test" and a.batch_size == 128 and a.seed == 42 and a.max_samples is None
    assert a.exp == "biomedclip_retrieval" and a.output_dir is None and a.save_features is False and a.mona_variant == "freq_enhanced"
    assert a.dtype == "bf16" and a.synthetic is False and a.synthetic_test == 64 and a.data_pt is None and a.ckpt_path is None and a.model_config is None
    assert a.device in ("cuda:0", "cpu")
    b = retrieval.get_args(["--k_values", "1", "5", "--split", "validation", "--save_features", "--dtype", "fp32"])
    assert b.k_values == [1, 5] and b.split == "validation" and b.save_features and b.dtype == "fp32"
    with pytest.raises(SystemExit):
        retrieval.get_args(["--split", "dev"])


def test_result_rows_follow_the_reference_order():
    from src.models.biomedclip import retrieval
    rows = retrieval.result_rows([1, 2], R.metrics(S4, (1, 2)))
    assert [r[0] for r in rows] == ["I2T_R@1", "I2T_R@2", "I2T_MedR", "I2T_MeanR", "T2I_R@1", "T2I_R@2", "T2I_MedR", "T2I_MeanR", "rSum"]
    assert [r[1] for r in rows] == [50.0, 75.0, 1.5, 1.75, 50.0, 75.0, 1.5, 2.0, 250.0]


# ------------------------------------------------------------------------------------------------ data module
def _dm_args(**kw):
    a = dict(data_pt=None, synthetic=True, synthetic_test=20, img_size=16, batch_size=8)
    a.update(kw)
    return SimpleNamespace(**a)


def test_synthetic_pairs_contract():
    from src.datasets.rocov2 import ROCOv2DataModule
    dm = ROCOv2DataModule(_dm_args(), cache_dir="unused", max_samples=None, seed=5)
    batches = list(dm.test_dataloader())
    assert [len(b[1]) for b in batches] == [8, 8, 4]
    images, captions, ids = batches[0]
    assert images.shape == (8, 3, 16, 16) and images.dtype == torch.float32 and 0.0 <= float(images.min()) and float(images.max()) < 1.0
    assert torch.equal(images[:, 0], images[:, 1]) and torch.equal(images[:, 0], images[:, 2])
    assert all(isinstance(c, str) and 4 <= len(c.split()) <= 11 for c in captions) and all(isinstance(i, str) for i in ids)
    assert captions[7] == captions[3] and len(set(ids)) == 8                   # duplicate captions are part of the contract
    again = list(ROCOv2DataModule(_dm_args(), cache_dir="unused", max_samples=None, seed=5).test_dataloader())
    assert all(torch.equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] for x, y in zip(batches, again))
    other = next(iter(ROCOv2DataModule(_dm_args(), cache_dir="unused", max_samples=None, seed=6).test_dataloader()))
    assert not torch.equal(other[0], images) and other[1] != captions
    tr, va = next(iter(dm.train_dataloader(shuffle=False))), next(iter(dm.val_dataloader()))
    assert not torch.equal(tr[0], images) and not torch.equal(va[0], images) and not torch.equal(tr[0], va[0])
    assert [b[2] for b in dm.train_dataloader(shuffle=False)] == [b[2] for b in dm.train_dataloader()]           # file order unless asked


def test_max_samples_truncates_every_split():
    from src.datasets.rocov2 import ROCOv2DataModule
    full = ROCOv2DataModule(_dm_args(), max_samples=None, seed=5)
    cut = ROCOv2DataModule(_dm_args(), max_samples=5, seed=5)
    for name in ("train_dataset", "val_dataset", "test_dataset"):
        a, b = getattr(full, name), getattr(cut, name)
        assert len(a) == 20 and len(b) == 5
        assert all(torch.equal(a[i][0], b[i][0]) and a[i][1:] == b[i][1:] for i in range(5))


def test_data_pt_pairs(tmp_path):
    from src.datasets.rocov2 import ROCOv2DataModule
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (10, 1, 16, 16), generator=g, dtype=torch.uint8)
    captions = [f"caption number {i}" for i in range(10)]
    path = tmp_path / "pairs.pt"
    torch.save({"images": images, "captions": captions}, path)
    dm = ROCOv2DataModule(_dm_args(synthetic=False, data_pt=str(path)), max_samples=None, seed=0)
    assert (len(dm.train_dataset), len(dm.val_dataset), len(dm.test_dataset)) == (7, 1, 2)
    im, cap, ids = next(iter(dm.test_dataloader()))
    assert im.shape == (2, 3, 16, 16) and cap == captions[8:] and ids == ["ROCOv2_000008", "ROCOv2_000009"]
    assert torch.equal(im[:, 0], images[8:, 0].float() / 255.0) and torch.equal(im[:, 0], im[:, 2])
    with pytest.raises(RuntimeError):
        ROCOv2DataModule(_dm_args(synthetic=False), max_samples=None, seed=0)
