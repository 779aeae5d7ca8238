"""-m gpu: the fused similarity-rank kernel (`uia_retrieval_ranks`, csrc/retrieval.hip) and `uia_retrieval_stats` against the float64 restatement of
tests/retrieval_reference.py: exact integer-valued features (every dot product exact in fp32 in any order, so the counts must be equal), normalised
real-valued features inside the worst-case bound of an fp32 fmaf chain, position independence, own-buffer hygiene, determinism, non-finite rows; then
compute_retrieval_metrics and the entry point src/models/biomedclip/retrieval.py."""
import csv
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import retrieval_reference as R  # noqa: E402
from guarded_out import PAD, dev  # noqa: E402

EXACT_SHAPES = [(1, 4), (97, 8), (333, 512), (1025, 16)]
REAL_SHAPES = [(97, 8, 1.5), (333, 72, 3.0)]
SENTINEL = -123456789


# ------------------------------------------------------------------------------------------------ cases (each reference computed once)
@functools.lru_cache(maxsize=None)
def exact_case(N, E):
    """Entries in {-3 .. 3}: |dot| <= 9 E <= 4608, exact in fp32.  img and txt are independent draws (nothing symmetric); planted, for N > 1: negative
    diagonals (txt_j = -img_j), identical text rows far apart (different 128-tiles when there is more than one), an all-zero image row and text row."""
    rng = np.random.default_rng(1000 * N + E)
    img = rng.integers(-3, 4, (N, E)).astype(np.float32)
    txt = rng.integers(-3, 4, (N, E)).astype(np.float32)
    if N > 1:
        for j in {1, N // 2, N - 2}:
            txt[j] = -img[j]
        txt[N - 1] = txt[0]
        txt[(2 * N) // 3] = txt[2]
        img[(2 * N) // 3 + 1] = img[4]
        img[3] = 0
        txt[5] = 0
    S = img.astype(np.float64) @ txt.astype(np.float64).T
    return img, txt, R.counts(S)


@functools.lru_cache(maxsize=None)
def real_case(N, E, noise):
    rng = np.random.default_rng(0)
    img = rng.standard_normal((N, E))
    txt = img + noise * rng.standard_normal((N, E))
    img, txt = img.astype(np.float32), txt.astype(np.float32)
    S = R.scores(img, txt, normalize=True)
    m = 4 * (E + 4) * 2.0 ** -24            # worst case of an E-term fp32 fmaf chain on unit vectors, four more terms for the normalisation
    return img, txt, R.counts(S, margin=m), R.counts(S, margin=-m)


def ranks(img, txt, normalize):
    from uia_hip import ops
    out = ops.retrieval_ranks(torch.from_numpy(np.ascontiguousarray(img)).to(dev()), torch.from_numpy(np.ascontiguousarray(txt)).to(dev()), normalize=normalize)
    return [o.cpu().numpy().astype(np.int64) for o in out]


NAMES = ("gt_i2t", "eq_i2t", "gt_t2i", "eq_t2i")


# ------------------------------------------------------------------------------------------------ exact counts
@pytest.mark.parametrize("N,E", EXACT_SHAPES)
def test_integer_features_give_exactly_the_reference_counts(N, E):
    img, txt, want = exact_case(N, E)
    got = ranks(img, txt, False)
    if N > 1:
        assert (np.diag(img.astype(np.float64) @ txt.astype(np.float64).T) < 0).sum() >= 2 and want[1].max() >= 1 and want[3].max() >= 1
        assert not np.array_equal(want[0], want[2])          # a transposed direction cannot pass
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (name, N, E, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


# ------------------------------------------------------------------------------------------------ normalised, real-valued
@pytest.mark.parametrize("N,E,noise", REAL_SHAPES)
def test_normalised_features_stay_inside_the_fp32_chain_bound(N, E, noise):
    img, txt, lo, hi = real_case(N, E, noise)
    got = ranks(img, txt, True)
    for d, (g, l, h) in (("i2t", (got[0], lo[0], hi[0])), ("t2i", (got[2], lo[2], hi[2]))):
        undecided = int((l != h).sum())
        print(f"N={N} E={E} {d}: {undecided} of {N} rows undecided by the reference, {int((g != l).sum())} rows differ from lo")
        assert undecided <= 0.02 * N, (d, undecided)
        assert ((l <= g) & (g <= h)).all(), (d, np.flatnonzero((g < l) | (g > h))[:8].tolist())
        assert (g[l == h] == l[l == h]).all(), d


def test_equal_rows_tie_exactly_wherever_they_fall():
    N, E, noise = REAL_SHAPES[1]
    img, txt, _, _ = real_case(N, E, noise)
    img, txt = img.copy(), txt.copy()
    img[300], txt[300] = img[5], txt[5]                       # tile 2 and tile 0, different lanes, waves and sub-tiles
    gt_r, eq_r, gt_c, eq_c = ranks(img, txt, True)
    assert gt_r[5] == gt_r[300] and gt_c[5] == gt_c[300]
    assert eq_r[5] >= 1 and eq_r[300] >= 1 and eq_c[5] >= 1 and eq_c[300] >= 1


# ------------------------------------------------------------------------------------------------ hygiene, determinism, non-finite
def test_outputs_and_workspace_may_be_uninitialised_and_guards_stay():
    from uia_hip import _lib, ops
    N, E = 333, 512
    img, txt, want = exact_case(N, E)
    a, b = torch.from_numpy(img).to(dev()), torch.from_numpy(txt).to(dev())
    lib = _lib.lib()
    need = lib.uia_retrieval_workspace_bytes(N, E)
    for normalize in (0, 1):
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev())
        bufs = [torch.full((PAD + N + PAD,), SENTINEL, dtype=torch.int32, device=dev()) for _ in range(4)]
        outs = [t[PAD:PAD + N] for t in bufs]
        _lib.check(lib.uia_retrieval_ranks(ops._stream(), N, E, a.data_ptr(), b.data_ptr(), normalize, ws.data_ptr(), need, *[o.data_ptr() for o in outs]),
                   "uia_retrieval_ranks")
        torch.cuda.synchronize()
        for t in bufs:
            h = t.cpu()
            assert bool((h[:PAD] == SENTINEL).all()) and bool((h[PAD + N:] == SENTINEL).all())
        assert bool((ws[need:].cpu() == 0xA5).all())
        if normalize == 0:
            for name, o, w in zip(NAMES, outs, want):
                assert np.array_equal(o.cpu().numpy().astype(np.int64), w), name
        else:
            clean = ranks(img, txt, True)
            for name, o, w in zip(NAMES, outs, clean):
                assert np.array_equal(o.cpu().numpy().astype(np.int64), w), name


def test_two_calls_agree_bit_for_bit():
    N, E, noise = REAL_SHAPES[1]
    img, txt, _, _ = real_case(N, E, noise)
    first, second = ranks(img, txt, True), ranks(img, txt, True)
    for name, x, y in zip(NAMES, first, second):
        assert np.array_equal(x, y), name
    img, txt, _ = exact_case(1025, 16)
    first, second = ranks(img, txt, False), ranks(img, txt, False)
    for name, x, y in zip(NAMES, first, second):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("normalize", [False, True])
def test_a_nan_row_ranks_last_and_counts_nowhere_else(normalize):
    N, E = 97, 8
    clean_img, txt, _ = exact_case(N, E)
    img = clean_img.copy()
    img[7, 2] = np.nan                                        # every score of image 7 is NaN, and so is d_7
    got = ranks(img, txt, normalize)
    assert got[0][7] == N - 1 and got[1][7] == 0 and got[2][7] == N - 1 and got[3][7] == 0
    keep = np.arange(N) != 7
    if not normalize:                                         # integer values: the restatement's IEEE comparisons give the counts exactly
        for name, g, w in zip(NAMES, got, R.counts(R.scores(img, txt, normalize=False))):
            assert np.array_equal(g, w), name
        return
    clean = ranks(clean_img, txt, True)
    # row i != 7 never meets image 7: unchanged.  Column j != 7 loses exactly what image 7 contributed to it, one greater or one equal at the most.
    assert np.array_equal(got[0][keep], clean[0][keep]) and np.array_equal(got[1][keep], clean[1][keep])
    lost_gt, lost_eq = clean[2][keep] - got[2][keep], clean[3][keep] - got[3][keep]
    assert ((lost_gt >= 0) & (lost_eq >= 0) & (lost_gt + lost_eq <= 1)).all()


# ------------------------------------------------------------------------------------------------ statistics
@functools.lru_cache(maxsize=None)
def stats_case(N, spread):
    rng = np.random.default_rng(77 + N)
    return rng.integers(0, (1 << 24) if spread else N, N).astype(np.int32)


@pytest.mark.parametrize("k_values", [(1, 2, 5, 10), (1,)])
@pytest.mark.parametrize("N,spread", [(1, False), (2, False), (7, False), (10000, False), (4097, True), (4098, True)])
def test_retrieval_stats_against_numpy(N, spread, k_values):
    from uia_hip import ops
    gt = stats_case(N, spread)
    rec = ops.retrieval_stats(torch.from_numpy(gt).to(dev()), k_values).cpu().tolist()
    want = R.stats(gt, k_values)
    assert len(rec) == len(k_values) + 2
    for k, g, w in zip(k_values, rec, want):
        assert abs(g - w) <= 1e-12, (N, k, g, w)
    assert rec[-2] == want[-2] and rec[-1] == want[-1], (N, rec[-2:], want[-2:])
    again = ops.retrieval_stats(torch.from_numpy(gt).to(dev()), k_values).cpu().tolist()
    assert again == rec


# ------------------------------------------------------------------------------------------------ Python surface
def _close(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        assert all(type(v) is float for v in got.values())
        if "r@" in k or k == "rsum":
            assert abs(got[k] - w) <= 1e-12 * max(1.0, abs(w)), (k, got[k], w)
        else:
            assert got[k] == w, (k, got[k], w)


def test_compute_retrieval_metrics_equals_the_restatement():
    from src.utils.retrieval_metrics import compute_retrieval_metrics
    img, txt, want = exact_case(333, 512)
    got = compute_retrieval_metrics(torch.from_numpy(img).to(dev()), torch.from_numpy(txt).to(dev()), k_values=(1, 5, 10), normalize=False)
    _close(got, R.metrics(want, (1, 5, 10)))
    assert got["n"] == 333.0 and got["i2t_ties"] >= 1 and got["t2i_ties"] >= 1


TOY_CFG = ("dict(embed_dim=128, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2), "
           "text_cfg=dict(vocab_size=30000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64))")


def _toy_mona_checkpoint(path):
    from src.adapters import inject_mona_variant_to_open_clip
    from src.utils.tools import parse_config
    from src.third_party.biomedclip.model import create_biomedclip
    model = create_biomedclip(config=parse_config(TOY_CFG), seed=42)
    inject_mona_variant_to_open_clip(model, variant="freq_enhanced", bottleneck_dim=64)
    g = torch.Generator().manual_seed(3)
    state = {k: v + 0.05 * torch.randn(v.shape, generator=g) for k, v in model.state_dict().items() if "mona" in k and v.is_floating_point()}
    assert state
    torch.save({"mona_state_dict": state}, path)


@pytest.mark.parametrize("mode", ["fp32", "mona"])
def test_entry_point_reports_what_its_saved_features_give(mode, tmp_path, monkeypatch):
    from src.models.biomedclip import retrieval
    from src.utils.retrieval_metrics import compute_retrieval_metrics
    from uia_hip import functional as UF
    monkeypatch.chdir(tmp_path)
    argv = ["--synthetic", "--synthetic_test", "48", "--batch_size", "16", "--k_values", "1", "5", "--img_size", "32", "--model_config", TOY_CFG,
            "--save_features", "--exp", "rt"]
    if mode == "fp32":
        argv += ["--dtype", "fp32"]
    else:
        _toy_mona_checkpoint(tmp_path / "mona.pth")
        argv += ["--mona_weights", str(tmp_path / "mona.pth")]
    try:
        metrics = retrieval.main(argv)
    finally:
        UF.set_compute_dtype(torch.bfloat16)
    folders = glob.glob(str(tmp_path / "runs" / "rt" / "test" / "*_rsum=*"))
    assert len(folders) == 1 and folders[0].endswith(f"_rsum={metrics['rsum']:.2f}")
    assert os.path.exists(os.path.join(folders[0], "log.log")) and not os.path.exists(tmp_path / "runs" / "rt" / "test" / "log.log")
    log = open(os.path.join(folders[0], "log.log")).read()
    assert "Image-to-Text Retrieval:" in log and "rSum:" in log and (mode == "fp32" or "MONA parameters from" in log)
    saved = torch.load(os.path.join(folders[0], "features.pth"))
    assert saved["image_features"].shape == (48, 128) and saved["text_features"].shape == (48, 128) and saved["image_features"].dtype == torch.float32
    assert len(saved["captions"]) == 48 and saved["captions"][7] == saved["captions"][3]
    again = compute_retrieval_metrics(saved["image_features"].to(dev()), saved["text_features"].to(dev()), k_values=[1, 5], normalize=True)
    assert again == metrics and saved["metrics"] == metrics
    _close(metrics, R.metrics(tuple(ranks(saved["image_features"].numpy(), saved["text_features"].numpy(), True)), (1, 5)))
    assert torch.equal(saved["text_features"][7], saved["text_features"][3])
    assert metrics["n"] == 48.0 and metrics["i2t_ties"] >= 12                  # duplicate captions: equal text features, so images 3 and 7, 11 and 15, .. see exact ties
    rows = list(csv.reader(open(os.path.join(folders[0], "results.csv"))))
    assert rows[0] == ["Metric", "Value"]
    assert [r[0] for r in rows[1:]] == ["I2T_R@1", "I2T_R@5", "I2T_MedR", "I2T_MeanR", "T2I_R@1", "T2I_R@5", "T2I_MedR", "T2I_MeanR", "rSum"]
    keys = ["i2t_r@1", "i2t_r@5", "i2t_medr", "i2t_meanr", "t2i_r@1", "t2i_r@5", "t2i_medr", "t2i_meanr", "rsum"]
    assert [r[1] for r in rows[1:]] == [f"{metrics[k]:.2f}" for k in keys]
