"""Host checks of the classification path: the float64 focal and metric restatements (tests/cls_reference.py) against closed forms, autograd and sklearn;
the four classification CLIs against the reference's argparse tables; the classification DataModule's batch and split contract; the loss module's
supported subset."""
import ast
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cls_reference as R  # noqa: E402


def _logits(N, C, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, generator=g, dtype=torch.float64) * scale, torch.randint(0, C, (N,), generator=g)


# ------------------------------------------------------------------------------------------------ focal restatement
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0, 3.7])
def test_focal_at_zero_logits_is_half_to_the_gamma_ln2(gamma):
    x = torch.zeros(5, 3, dtype=torch.float64)
    lab = torch.tensor([0, 1, 2, 1, 0])
    el = R.focal_elements(x, lab, gamma)
    assert torch.allclose(el, torch.full_like(el, 0.5 ** gamma * math.log(2.0)), rtol=1e-15, atol=0)
    assert abs(float(R.focal_loss(x, lab, gamma)) - 0.5 ** gamma * math.log(2.0)) < 1e-15


def test_focal_with_gamma_zero_is_bce_with_logits():
    x, lab = _logits(37, 5, 1)
    want = F.binary_cross_entropy_with_logits(x, F.one_hot(lab, 5).double())
    assert abs(float(R.focal_loss(x, lab, 0.0)) - float(want)) < 1e-14


@pytest.mark.parametrize("alpha", [0.25, 0.8])
def test_focal_alpha_weights_targets_by_alpha_and_the_rest_by_one_minus_alpha(alpha):
    x, lab = _logits(19, 4, 2)
    base = R.focal_elements(x, lab, 2.0)
    t = F.one_hot(lab, 4).bool()
    got = R.focal_elements(x, lab, 2.0, alpha)
    assert torch.allclose(got[t], alpha * base[t], rtol=1e-14) and torch.allclose(got[~t], (1 - alpha) * base[~t], rtol=1e-14)


@pytest.mark.parametrize("gamma,alpha", [(0.0, None), (2.0, None), (3.7, 0.25), (0.5, 0.9)])
def test_focal_closed_form_gradient_matches_autograd(gamma, alpha):
    x, lab = _logits(23, 6, 3)
    x = torch.cat([x, torch.tensor([[100.0, -100.0, 30.0, -30.0, 0.0, 1e-3]], dtype=torch.float64)])
    lab = torch.cat([lab, torch.tensor([1])])
    xr = x.clone().requires_grad_(True)
    R.focal_loss(xr, lab, gamma, alpha).backward()
    got = R.focal_grad(x, lab, gamma, alpha)
    assert torch.isfinite(got).all()
    assert float((got - xr.grad).abs().max()) <= 1e-15 + 1e-12 * float(xr.grad.abs().max())


def test_focal_restatement_is_finite_at_100():
    x = torch.tensor([[100.0, -100.0], [-100.0, 100.0]], dtype=torch.float64)
    lab = torch.tensor([0, 0])
    assert math.isfinite(float(R.focal_loss(x, lab, 2.0)))
    assert abs(float(R.focal_elements(x, lab, 2.0)[1, 1]) - 100.0) < 1e-9      # a confident wrong logit: σ(100)^2 · softplus(100)


# ------------------------------------------------------------------------------------------------ metrics restatement vs sklearn
def _sk(p1, y):
    from sklearn.metrics import accuracy_score, f1_score, precision_score, recall_score, roc_auc_score
    pred = (np.asarray(p1, np.float32) > np.float32(0.5)).astype(int)
    out = dict(acc=accuracy_score(y, pred), pre=precision_score(y, pred, zero_division=0), rec=recall_score(y, pred, zero_division=0),
               f1=f1_score(y, pred, zero_division=0))
    out["auc"] = roc_auc_score(y, p1) if len(set(np.asarray(y).tolist())) == 2 else 0.0
    return out


def _cases():
    rs = np.random.RandomState(0)
    yield "random", rs.rand(500).astype(np.float32), rs.randint(0, 2, 500)
    yield "heavy ties", (rs.randint(0, 5, 400) / 4.0).astype(np.float32), rs.randint(0, 2, 400)
    yield "all equal", np.full(50, 0.3, np.float32), np.r_[np.zeros(20, int), np.ones(30, int)]
    yield "one class absent", rs.rand(40).astype(np.float32), np.ones(40, int)
    yield "only negatives", rs.rand(40).astype(np.float32), np.zeros(40, int)
    yield "exactly one half", np.array([0.5, 0.5, 0.5000001, 0.4999999, 0.7, 0.2], np.float32), np.array([1, 0, 1, 0, 1, 0])
    yield "single", np.array([0.9], np.float32), np.array([1])
    yield "separable", np.linspace(0, 1, 64).astype(np.float32), (np.arange(64) >= 32).astype(int)


@pytest.mark.parametrize("name,p1,y", list(_cases()), ids=[c[0] for c in _cases()])
def test_metric_restatement_matches_sklearn(name, p1, y):
    from src.utils.cls_metrics import metrics_from_counts
    tp, fp, tn, fn, auc = R.binary_stats(p1, y)
    got = metrics_from_counts(tp, fp, tn, fn)
    want = _sk(p1, y)
    for k in ("acc", "pre", "rec", "f1"):
        assert abs(got[k] - want[k]) < 1e-15, (k, got[k], want[k])
    assert abs(auc - want["auc"]) < 1e-12, (auc, want["auc"])
    if name == "all equal":
        assert auc == 0.5
    if name in ("one class absent", "only negatives"):
        assert auc == 0.0
    if name == "exactly one half":
        assert (tp, fp, tn, fn) == (2.0, 0.0, 3.0, 1.0)               # p1 == 0.5 counts as predicted negative


def test_classification_metrics_refuse_more_than_two_classes_and_seg_accumulator_still_refuses_cls():
    from src.utils.cls_metrics import ClassificationMetrics
    from src.utils.tools import MetricAccumulator
    with pytest.raises(NotImplementedError):
        ClassificationMetrics(num_classes=3)
    with pytest.raises(NotImplementedError):
        MetricAccumulator(type="cls")
    assert all(math.isnan(v) for v in ClassificationMetrics().compute().values())


# ------------------------------------------------------------------------------------------------ FocalLoss surface
def test_focal_loss_module_supports_the_reference_subset_only():
    from src.losses import FocalLoss
    f = FocalLoss(to_onehot_y=True)
    assert f.gamma == 2.0 and f.alpha is None
    assert FocalLoss(to_onehot_y=True, gamma=0.5, alpha=0.25).alpha == 0.25
    for kw in (dict(), dict(to_onehot_y=True, use_softmax=True), dict(to_onehot_y=True, reduction="sum"), dict(to_onehot_y=True, reduction="none"),
               dict(to_onehot_y=True, include_background=False), dict(to_onehot_y=True, weight=[1.0, 2.0])):
        with pytest.raises(NotImplementedError):
            FocalLoss(**kw)


# ------------------------------------------------------------------------------------------------ CLI tables
ENTRIES = ["biomedclip/classification.py", "clip/classification.py", "metaclip/classification.py", "unimedclip/classification.py"]
ADDITIONS = ["--dtype", "--synthetic", "--synthetic_train", "--synthetic_val", "--synthetic_test", "--data_pt", "--ckpt_path", "--model_config",
             "--extract_layers", "--val_every", "--stats_json"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_classification_cli_carries_every_reference_flag_and_default(entry):
    import importlib
    from oracle.gen_host_fixtures import argparse_table
    ref = json.load(open(os.path.join(HERE, "golden", "reference_cls_cli_tables.json")))[entry]
    assert len(ref) >= 25
    got = argparse_table(os.path.join(ROOT, "nextgen-uia_amd/src/models", entry))
    mod = importlib.import_module("src.models." + entry[:-3].replace("/", "."))
    args = vars(mod.get_args([]))
    for flag, kw in ref.items():
        assert flag in got, (entry, flag)
        if flag == "--device":
            continue
        assert got[flag] == kw, (entry, flag, kw, got[flag])
        if "default" in kw:
            assert args[flag[2:]] == ast.literal_eval(kw["default"]), (entry, flag)
    for flag in ADDITIONS:
        assert flag[2:] in args, (entry, flag)
    assert args["val_every"] == 10 and args["extract_layers"] == "3,6,9"


# ------------------------------------------------------------------------------------------------ DataModule
def _dm_args(**kw):
    a = dict(data_pt=None, synthetic=True, synthetic_train=20, synthetic_val=6, synthetic_test=8, img_size=32, seed=3, batch_size=4)
    a.update(kw)
    return SimpleNamespace(**a)


def test_synthetic_classes_are_balanced_deterministic_and_separable():
    from src.datasets import classification as D
    a, b = D.DataModule(_dm_args()), D.DataModule(_dm_args())
    assert len(a.train_dataset) == 20 and len(a.val_dataset) == 6 and len(a.test_dataset) == 8
    assert torch.equal(a.train_dataset.images, b.train_dataset.images) and torch.equal(a.train_dataset.labels, b.train_dataset.labels)
    assert not torch.equal(a.train_dataset.images, a.val_dataset.images[:1].expand(20, -1, -1, -1))
    lab = a.train_dataset.labels
    assert int(lab.sum()) == 10
    img = a.train_dataset.images
    assert float(img.min()) >= 0 and float(img.max()) <= 1
    bright = (img > 0.85).flatten(1).float().mean(1)                # the lesion: class 1 only
    assert float(bright[lab == 0].max()) == 0.0 and float(bright[lab == 1].min()) > 0.01


def test_batches_follow_the_contract_and_splits_default_to_70_10_20(tmp_path):
    from src.datasets import classification as D
    dm = D.DataModule(_dm_args())
    tl = dm.train_dataloader()
    batches = list(tl)
    assert len(batches) == 5 and all(len(b[0]) == 4 for b in batches)               # drop_last on the training split
    images, labels, names = batches[0]
    assert images.dtype == torch.float32 and tuple(images.shape) == (4, 1, 32, 32)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (4,) and len(names) == 4
    assert [len(b[0]) for b in dm.test_dataloader()] == [4, 4] and [len(b[0]) for b in dm.val_dataloader()] == [4, 2]
    assert D.second_of(batches[0]) is labels
    n = 50
    blob = {"images": torch.randint(0, 256, (n, 3, 16, 16), dtype=torch.uint8), "labels": torch.arange(n) % 2}
    torch.save(blob, tmp_path / "d.pt")
    dm = D.DataModule(_dm_args(data_pt=str(tmp_path / "d.pt"), synthetic=False, batch_size=8))
    assert (len(dm.train_dataset), len(dm.val_dataset), len(dm.test_dataset)) == (35, 5, 10)
    im, lab, nm = dm.test_dataset[0]
    assert tuple(im.shape) == (1, 16, 16) and torch.equal(im, blob["images"][40, :1].float() / 255) and int(lab) == 0 and nm == "00040.png"
    blob["split"] = {"train": [1, 2, 3], "val": [4], "test": [0, 5]}
    blob["names"] = [f"img{i}" for i in range(n)]
    torch.save(blob, tmp_path / "e.pt")
    dm = D.DataModule(_dm_args(data_pt=str(tmp_path / "e.pt"), synthetic=False))
    assert dm.test_dataset.names == ["img0", "img5"] and len(dm.train_dataset) == 3
    with pytest.raises(RuntimeError):
        D.DataModule(_dm_args(synthetic=False))
