"""GPU checks of zero-shot classification: uia_zero_shot_score against the float64 restatement mean_p(100 · f̂ · t̂_p) (tests/zero_shot_reference.py), its
position independence bit for bit, its edge contract; uia_binary_roc_curve against the numpy restatement and the AUROC of uia_binary_cls_stats; the four
entry points and the post-training evaluation of the MetaCLIP fine-tune entry."""
import csv
import glob
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

import zero_shot_reference as Z  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = {"10+10": (10, 10), "10+7": (10, 7), "11+11+11": (11, 11, 11)}


def _offsets(layout):
    return [0] + list(np.cumsum(layout))


def _features(N, T, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, E, generator=g) * 3.0, torch.randn(T, E, generator=g) * 0.5 + 0.1       # raw tower outputs: neither unit norm nor centred


# ------------------------------------------------------------------------------------------------ 1. scoring against float64
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("E", [50, 512, 768])
def test_scores_probs_and_normalised_rows_against_float64(E, layout):
    """|logit - float64| <= 100·(2E+16)·2^-24 (derived: tests/zero_shot_reference.logit_bound), probs within 4 fp32 ulp of the float64 softmax of the kernel's
    own logits, img_n rows of unit norm within (E+8)·2^-24.  Observed logit error (MI355X): 2.8e-6 at worst over every case (printed below)."""
    from uia_hip import ops
    off = _offsets(LAYOUTS[layout])
    worst = 0.0
    for N in (1, 31, 33, 70):
        img, prm = _features(N, off[-1], E, seed=1000 + N + E)
        logits, probs, img_n = ops.zero_shot_score(img.cuda(), prm.cuda(), off, want_normalized=True)
        assert logits.shape == (N, len(off) - 1) and probs.shape == logits.shape and img_n.shape == (N, E)
        lg = logits.cpu().numpy()
        err = float(np.abs(lg.astype(np.float64) - Z.score(img.numpy(), prm.numpy(), off)).max())
        worst = max(worst, err)
        assert err <= Z.logit_bound(E), (N, E, layout, err, Z.logit_bound(E))
        want = Z.softmax(lg)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(probs.cpu().numpy().astype(np.float64) - want) <= 4 * ulp), (N, E, layout)
        nrm = np.linalg.norm(img_n.cpu().numpy().astype(np.float64), axis=1)
        assert np.all(np.abs(nrm - 1.0) <= (E + 8) * 2.0 ** -24), (N, E, layout, float(np.abs(nrm - 1.0).max()))
    print(f"zero_shot_score E={E} layout={layout}: max |logit error| {worst:.3e} (bound {Z.logit_bound(E):.3e})")


def test_probs_stay_finite_for_logits_of_plus_minus_100():
    """Image rows equal to ± one prompt direction: logits of about +100 / -100, probabilities exactly representable ends of the range."""
    from uia_hip import ops
    E = 64
    g = torch.Generator().manual_seed(3)
    d = torch.randn(E, generator=g)
    prm = torch.cat([d.repeat(10, 1), (-d).repeat(10, 1)])
    img = torch.stack([d, -d, 2.5 * d])
    logits, probs, _ = ops.zero_shot_score(img.cuda(), prm.cuda(), [0, 10, 20])
    lg, pr = logits.cpu().numpy(), probs.cpu().numpy()
    assert np.all(np.abs(np.abs(lg) - 100.0) < 1e-3) and lg[0, 0] > 0 > lg[0, 1] and lg[1, 1] > 0 > lg[1, 0]
    assert np.all(np.isfinite(pr)) and np.array_equal(pr, np.array([[1, 0], [0, 1], [1, 0]], np.float32))


# ------------------------------------------------------------------------------------------------ 2. position independence
@pytest.mark.parametrize("layout", ["10+10", "11+11+11"])
def test_logits_do_not_depend_on_the_batching_bit_for_bit(layout):
    from uia_hip import ops
    off = _offsets(LAYOUTS[layout])
    C = len(off) - 1
    img, prm = _features(70, off[-1], 512, seed=7)
    img, prm = img.cuda(), prm.cuda()
    whole, whole_p, whole_n = ops.zero_shot_score(img, prm, off, want_normalized=True)
    buf = torch.full((70, C), float("nan"), device="cuda")
    parts_p, parts_n = [], []
    for r0, r1 in ((0, 32), (32, 64), (64, 70)):
        _, p, n = ops.zero_shot_score(img[r0:r1], prm, off, out=buf, row=r0, want_normalized=True)
        parts_p.append(p)
        parts_n.append(n)
    rev, rev_p, _ = ops.zero_shot_score(img.flip(0), prm, off)
    assert torch.equal(whole.view(torch.int32), buf.view(torch.int32))
    assert torch.equal(whole.view(torch.int32), rev.flip(0).contiguous().view(torch.int32))
    assert torch.equal(whole_p.view(torch.int32), torch.cat(parts_p).view(torch.int32)) and torch.equal(whole_p, rev_p.flip(0))
    assert torch.equal(whole_n.view(torch.int32), torch.cat(parts_n).view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. edges
def test_zero_rows_poison_only_their_own_row_or_class():
    from uia_hip import ops
    off = _offsets((11, 11, 11))
    img, prm = _features(40, 33, 50, seed=11)
    clean, _, _ = ops.zero_shot_score(img.cuda(), prm.cuda(), off)
    img0 = img.clone()
    img0[33] = 0.0
    a, pa, _ = ops.zero_shot_score(img0.cuda(), prm.cuda(), off)
    keep = torch.arange(40) != 33
    assert bool(torch.isnan(a[33]).all()) and bool(torch.isnan(pa[33]).all())
    assert torch.equal(a.cpu()[keep], clean.cpu()[keep]) and bool(torch.isfinite(pa.cpu()[keep]).all())
    prm0 = prm.clone()
    prm0[15] = 0.0                                               # a prompt of class 1
    b, _, _ = ops.zero_shot_score(img.cuda(), prm0.cuda(), off)
    assert bool(torch.isnan(b[:, 1]).all())
    assert torch.equal(b.cpu()[:, [0, 2]], clean.cpu()[:, [0, 2]])


def test_logits_are_written_only_inside_their_rows():
    from uia_hip import ops
    off = _offsets((10, 7))
    img, prm = _features(33, 17, 50, seed=13)
    canary = -12345.5
    buf = torch.full((80, 2), canary, device="cuda")
    view, _, _ = ops.zero_shot_score(img.cuda(), prm.cuda(), off, out=buf, row=20)
    alone, _, _ = ops.zero_shot_score(img.cuda(), prm.cuda(), off)
    assert view.data_ptr() == buf[20:].data_ptr() and torch.equal(buf[20:53], alone)
    assert bool((buf[:20] == canary).all()) and bool((buf[53:] == canary).all())


def test_limit_violations_are_refused_with_a_message_and_launch_nothing():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    canary = 7.25
    img = torch.randn(4, 16).cuda()

    def refused(off, E=16, text="uia_zero_shot_score"):
        out = torch.full((4, len(off) - 1), canary, device="cuda")
        with pytest.raises(UiaError) as e:
            ops.zero_shot_score(img[:, :E], torch.randn(off[-1], E).cuda(), off, out=out)
        assert text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert bool((out == canary).all())

    refused([0, 5], text="C=1")                                              # C = 1
    refused(list(range(0, 10)), text="C=9")                                  # C = 9, one prompt each
    refused([0, 33, 40], text="33 prompts")                                  # 33 prompts in a class
    refused([0] + [32 * (c + 1) for c in range(7)] + [257], text="T=257")    # T = 257 (8 classes, the last with 33: T is named first)
    refused([0, 10, 20], E=0, text="E=0")                                    # E = 0
    # the largest legal layout is not refused: 8 classes of 32 prompts, T = 256
    prm = torch.randn(256, 16)
    full, _, _ = ops.zero_shot_score(img, prm.cuda(), [32 * c for c in range(9)])
    ref = Z.score(img.cpu().numpy(), prm.numpy(), [32 * c for c in range(9)])
    assert float(np.abs(full.cpu().numpy() - ref).max()) <= Z.logit_bound(16)


# ------------------------------------------------------------------------------------------------ 4. ROC curve
def _roc(p, y):
    from uia_hip import ops
    count, fpr, tpr, thr = ops.binary_roc_curve(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())
    n = int(count.item())
    return n, fpr.cpu().numpy(), tpr.cpu().numpy(), thr.cpu().numpy()


@pytest.mark.parametrize("tied", [True, False], ids=["seven_values", "all_distinct"])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000])
def test_roc_curve_against_the_restatement_and_the_auroc(N, tied):
    from uia_hip import ops
    p, y = Z.roc_inputs(N, tied, seed=N)
    n, fpr, tpr, thr = _roc(p, y)
    rf, rt, rthr = Z.roc_curve(p, y)
    assert n == len(rthr) and (n == min(N, 7) + 1 if tied and N >= 255 else n <= N + 1)
    assert np.array_equal(thr[:n], rthr) and np.array_equal(fpr[:n], rf) and np.array_equal(tpr[:n], rt)      # exact: ratios of the same integers
    assert not fpr[n:].any() and not tpr[n:].any() and not thr[n:].any()                                      # past count: left as they were
    area = float(np.sum((fpr[1:n] - fpr[:n - 1]) * (tpr[1:n] + tpr[:n - 1]) * 0.5))
    auc = float(ops.binary_cls_stats(torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda())[4])
    assert abs(area - auc) <= 1e-12, (N, tied, area, auc)


@pytest.mark.parametrize("label", [0, 1])
def test_roc_curve_with_one_class_absent_has_an_all_zero_axis(label):
    p, _ = Z.roc_inputs(257, True, seed=5)
    y = np.full(257, label, np.int64)
    n, fpr, tpr, thr = _roc(p, y)
    rf, rt, rthr = Z.roc_curve(p, y)
    assert n == 8 and np.array_equal(thr[:n], rthr) and np.array_equal(fpr[:n], rf) and np.array_equal(tpr[:n], rt)
    assert not (fpr if label == 1 else tpr)[:n].any() and (tpr if label == 1 else fpr)[n - 1] == 1.0


def test_roc_curve_refuses_bad_labels_and_nan_scores():
    p, y = Z.roc_inputs(300, False, seed=9)
    y2 = y.copy()
    y2[123] = 2
    n, fpr, tpr, thr = _roc(p, y2)
    assert n == -1 and not fpr.any() and not tpr.any() and not thr.any()     # the arrays are left unwritten
    p2 = p.copy()
    p2[7] = np.nan
    n, fpr, tpr, thr = _roc(p2, y)
    assert n == -1 and not fpr.any() and not tpr.any() and not thr.any()


# ------------------------------------------------------------------------------------------------ 5. entry points
BIOMED_TOY = ("dict(embed_dim=128, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2), "
              "text_cfg=dict(vocab_size=30000, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, max_position_embeddings=64))")
METACLIP_TOY = ("dict(embed_dim=128, vision_cfg=dict(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2, eps=1e-5, "
                "act='quick_gelu', pre_norm=True, patch_bias=False), "
                "text_cfg=dict(context_length=16, vocab_size=4000, width=128, heads=2, layers=2, act='quick_gelu'))")
CLIP_TOY = "(64, 32, 2, 128, 8, 16, 4000, 128, 2, 2)"
UNIMED_TOY = "dict(embed_dim=64, image_size=32, vision_layers=2, vision_width=128, patch_size=8, context_length=16, vocab_size=30522, width=64, heads=2, layers=1)"
FAMILIES = {"biomedclip": ["--model_config", BIOMED_TOY], "metaclip": ["--model_config", METACLIP_TOY], "clip": ["--model_config", CLIP_TOY, "--ckpt", ""],
            "unimedclip": ["--model_config", UNIMED_TOY, "--ckpt", ""]}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_entry_point_writes_the_report_and_does_not_depend_on_the_batch_size(family, tmp_path, monkeypatch):
    import importlib
    from src.models import zero_shot_eval as ZS
    from uia_hip import ops
    mod = importlib.import_module(f"src.models.{family}.zero_shot")
    monkeypatch.chdir(tmp_path)
    common = ["--synthetic", "--synthetic_test", "40", "--img_size", "32", "--dtype", "fp32"] + FAMILIES[family]
    argv = common + ["--exp", "a", "--batch_size", "16"]
    stats = mod.main(argv)
    folder = stats["report_dir"]
    assert os.path.dirname(folder) == os.path.join("runs", "a", "LN-INT", "test") and os.path.exists(os.path.join("runs", "a", "LN-INT", "test", "results.json"))
    rows = list(csv.reader(open(os.path.join(folder, "results.csv"))))
    assert rows[0] == ["Metric", "Mean"] and [r[0] for r in rows[1:]] == ["Acc", "Rec", "Pre", "F1", "AUC"]
    assert all(r[1] == f"{float(r[1]):.2f}" and 0.0 <= float(r[1]) <= 100.0 for r in rows[1:])
    assert os.path.exists(os.path.join(folder, "log.log"))
    # the returned logits give the folder's accuracy and the curve's point count
    args = mod.get_args(argv)
    stats2, logits = mod.test(args)
    labels = ZS.load_test_split(args)[1]
    assert tuple(logits.shape) == (40, 2) and not logits.is_cuda and bool(torch.isfinite(logits).all()) and stats2["n"] == 40
    acc = int((logits.argmax(1) == labels).sum()) / 40
    assert folder.endswith(f"_acc={acc * 100:.2f}") and rows[1][1] == f"{acc * 100:.2f}" and stats["acc"] == acc
    count = int(ops.binary_roc_curve(torch.softmax(logits.cuda(), dim=1)[:, 1], labels.cuda())[0].item())
    roc = list(csv.reader(open(os.path.join(folder, "roc_curve.csv"))))
    assert roc[0] == ["fpr", "tpr", "threshold"] and len(roc) - 1 == count and 2 <= count <= 41
    assert [float(v) for v in roc[1]] == [0.0, 0.0, 1.0] and float(roc[-1][0]) == 1.0 and float(roc[-1][1]) == 1.0
    try:
        import matplotlib  # noqa: F401
        assert os.path.exists(os.path.join(folder, f"roc_curve_{family}_zero_shot.png"))
    except ImportError:
        pass
    # one batch of 40 instead of 16 + 16 + 8: the same bytes
    other = mod.main(common + ["--exp", "b", "--batch_size", "40"])["report_dir"]
    for name in ("results.csv", "roc_curve.csv"):
        assert open(os.path.join(folder, name), "rb").read() == open(os.path.join(other, name), "rb").read(), name


def test_metaclip_finetune_zero_shot_eval_runs_the_three_evaluations(tmp_path, monkeypatch):
    """--zero_shot_eval: after two tiny epochs rank 0 starts metaclip/zero_shot.py on best_model.pth once per dataset, each a child process."""
    from src.models.metaclip import finetune
    monkeypatch.chdir(tmp_path)
    out = finetune.main(["--synthetic", "--synthetic_train", "32", "--synthetic_val", "16", "--img_size", "32", "--batch_size", "16", "--epochs", "2", "--lr", "2e-3",
                         "--dtype", "bf16", "--exp", "m", "--model_config", METACLIP_TOY, "--num_workers", "0", "--zero_shot_eval", "--zero_shot_timeout", "300"])
    assert out["zero_shot"] == ["LN-INT", "LN-EXT", "BUSI"], open(tmp_path / "runs" / "m" / "log.log").read()[-3000:]
    for dataset in out["zero_shot"]:
        found = glob.glob(str(tmp_path / "runs" / "m" / dataset / "test" / "*_acc=*" / "results.csv"))
        assert len(found) == 1, (dataset, found)
        assert os.path.exists(os.path.join(os.path.dirname(found[0]), "roc_curve.csv"))
    assert math.isfinite(out["best_val"])
