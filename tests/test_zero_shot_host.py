"""Host checks of zero-shot classification: the argparse tables of the three new entry points against the reference's (data:
tests/golden/reference_cli_tables_zero_shot.json), the ROC restatement of tests/zero_shot_reference.py against scikit-learn, the new C entries' presence and
their argument checks (which fail before any launch), and the host helpers of src/models/zero_shot_eval.py."""
import ast
import ctypes
import json
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

GOLDEN_TABLES = os.path.join(HERE, "golden", "reference_cli_tables_zero_shot.json")
ENTRIES = ["metaclip/zero_shot.py", "clip/zero_shot.py", "unimedclip/zero_shot.py"]


# ------------------------------------------------------------------------------------------------ command lines
def _argparse_table(path):
    """Flag -> {default, action, choices} as source expressions: the walk of tests/test_round6_host.py."""
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument" and node.args and isinstance(node.args[0], ast.Constant):
            out[node.args[0].value] = {k.arg: ast.unparse(k.value) for k in node.keywords if k.arg in ("default", "action", "choices")}
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_reference_flag_is_there_with_its_default(entry):
    """Flag set and default / action / choices expressions compared syntactically; `--device` is the one deliberate difference (decided without a HIP
    call, src/utils/tools.default_device)."""
    ref = json.load(open(GOLDEN_TABLES))[entry]
    got = _argparse_table(os.path.join(ROOT, "nextgen-uia_amd/src/models", entry))
    assert ref and "--mona_weights" in ref and "--batch_size" in ref, entry
    for flag, kw in ref.items():
        assert flag in got, (entry, flag)
        if flag != "--device":
            assert got[flag] == kw, (entry, flag, kw, got[flag])


@pytest.mark.parametrize("family", ["metaclip", "clip", "unimedclip", "biomedclip"])
def test_entry_points_carry_the_build_flags_and_parse_without_a_gpu(family):
    import importlib
    mod = importlib.import_module(f"src.models.{family}.zero_shot")
    a = mod.get_args([])
    assert (a.dtype, a.synthetic, a.synthetic_test, a.data_pt, a.prompts_json, a.ckpt_path, a.model_config) == ("bf16", False, 64, None, None, None, None)
    assert a.exp == f"{family}_zero_shot" and a.dataset == "LN-INT" and a.batch_size == 32 and a.num_classes == 2
    b = mod.get_args(["--synthetic", "--synthetic_test", "40", "--dtype", "fp32", "--batch_size", "16"])
    assert b.synthetic and b.synthetic_test == 40 and b.dtype == "fp32" and b.batch_size == 16


@pytest.mark.parametrize("family", ["metaclip", "clip", "unimedclip"])
def test_zero_shot_eval_is_off_by_default_on_the_finetune_entries(family):
    import importlib
    mod = importlib.import_module(f"src.models.{family}.finetune")
    a = mod.get_args([])
    assert a.zero_shot_eval is False and a.zero_shot_data_pt is None and a.zero_shot_timeout > 0
    assert mod.get_args(["--zero_shot_eval"]).zero_shot_eval is True


def test_a_failed_child_ends_the_post_training_evaluation(tmp_path, monkeypatch):
    """run_zero_shot_evaluation: a fresh child per dataset (sys.executable, a timeout); the first failure is logged and no further dataset is started."""
    import subprocess
    from src.models import contrastive as F
    from src.models.metaclip import finetune as entry
    script = entry.RECIPE.zero_shot_script
    monkeypatch.chdir(tmp_path)
    args = entry.get_args(["--exp", "x", "--synthetic", "--zero_shot_eval", "--zero_shot_timeout", "7"])
    args.train_snapshot_path = str(tmp_path)
    assert F.run_zero_shot_evaluation(args, script) == []                    # no best_model.pth: nothing is started
    torch.save({}, tmp_path / "best_model.pth")
    calls = []

    def fake_run(cmd, **kw):
        calls.append((cmd, kw))
        return subprocess.CompletedProcess(cmd, 0 if len(calls) == 1 else 3, stdout="", stderr="boom")

    monkeypatch.setattr(F.subprocess, "run", fake_run)
    assert F.run_zero_shot_evaluation(args, script, extra=["--ckpt_path", "w.pt"]) == ["LN-INT"]
    assert len(calls) == 2                                                   # LN-EXT failed: BUSI is never started
    cmd, kw = calls[0]
    assert cmd[0] == sys.executable and cmd[1].endswith(os.path.join("metaclip", "zero_shot.py")) and kw["timeout"] == 7
    for flag, value in (("--exp", "x"), ("--dataset", "LN-INT"), ("--img_size", "224"), ("--mona_weights", str(tmp_path / "best_model.pth")),
                        ("--mona_bottleneck", "64"), ("--batch_size", "64"), ("--seed", "1"), ("--dtype", "bf16"), ("--ckpt_path", "w.pt")):
        assert cmd[cmd.index(flag) + 1] == value, flag
    assert "--synthetic" in cmd and "--data_pt" not in cmd and calls[1][0][calls[1][0].index("--dataset") + 1] == "LN-EXT"

    def slow_run(cmd, **kw):
        calls.append((cmd, kw))
        raise subprocess.TimeoutExpired(cmd, kw["timeout"])

    del calls[:]
    monkeypatch.setattr(F.subprocess, "run", slow_run)
    assert F.run_zero_shot_evaluation(args, script) == [] and len(calls) == 1


# ------------------------------------------------------------------------------------------------ the ROC restatement
@pytest.mark.parametrize("tied", [True, False], ids=["seven_values", "all_distinct"])
@pytest.mark.parametrize("N", [2, 255, 256, 257, 1000])
def test_roc_restatement_agrees_with_scikit_learn(N, tied):
    metrics = pytest.importorskip("sklearn.metrics")
    p, y = Z.roc_inputs(N, tied, seed=N)
    fpr, tpr, thr = Z.roc_curve(p, y)
    sf, st, sthr = metrics.roc_curve(y, p, drop_intermediate=False)
    assert len(fpr) == len(sf) and np.array_equal(fpr, sf) and np.array_equal(tpr, st)
    assert np.isinf(sthr[0]) and thr[0] == 1.0                               # the one difference: scikit-learn opens with inf, torchmetrics (and we) with 1.0
    assert np.array_equal(thr[1:], sthr[1:].astype(np.float32))


@pytest.mark.parametrize("tied", [True, False], ids=["seven_values", "all_distinct"])
def test_roc_restatement_with_one_sample_keeps_the_absent_axis_at_zero(tied):
    """N = 1 has one class only: scikit-learn divides by zero on the absent class's axis (NaN, with a warning); torchmetrics, and we, leave it 0."""
    import warnings
    metrics = pytest.importorskip("sklearn.metrics")
    p, y = Z.roc_inputs(1, tied, seed=1)
    fpr, tpr, thr = Z.roc_curve(p, y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sf, st, sthr = metrics.roc_curve(y, p, drop_intermediate=False)
    present, absent, s_present, s_absent = (tpr, fpr, st, sf) if y[0] == 1 else (fpr, tpr, sf, st)
    assert np.array_equal(present, s_present) and present.tolist() == [0.0, 1.0]
    assert np.isnan(s_absent).all() and absent.tolist() == [0.0, 0.0]
    assert thr.tolist() == [1.0, p[0]] and np.isinf(sthr[0]) and sthr[1] == p[0]


def test_roc_restatement_by_hand():
    fpr, tpr, thr = Z.roc_curve(np.array([0.2, 0.7, 0.7, 0.4], np.float32), np.array([0, 1, 0, 1]))
    assert thr.tolist() == [1.0, np.float32(0.7), np.float32(0.4), np.float32(0.2)]
    assert fpr.tolist() == [0.0, 0.5, 0.5, 1.0] and tpr.tolist() == [0.0, 0.5, 1.0, 1.0]
    fpr, tpr, _ = Z.roc_curve(np.array([0.1, 0.9], np.float32), np.array([1, 1]))
    assert fpr.tolist() == [0.0, 0.0, 0.0] and tpr.tolist() == [0.0, 0.5, 1.0]


# ------------------------------------------------------------------------------------------------ the C entries without a GPU
NEW_SYMBOLS = ("uia_zero_shot_score", "uia_binary_roc_curve_workspace_bytes", "uia_binary_roc_curve")


def test_new_entries_are_declared_exported_typed_and_importable():
    from uia_hip import _lib, ops
    src = open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in src and hasattr(handle, name) and name in _lib.PROTOTYPES and name in doc, name
    assert callable(ops.zero_shot_score) and callable(ops.binary_roc_curve)
    from src.models import zero_shot_eval  # noqa: F401
    from src.utils.cls_metrics import ClassificationMetrics
    assert callable(ClassificationMetrics.roc)


def test_score_argument_checks_fail_before_any_launch():
    from uia_hip import _lib
    lib = _lib.lib()
    fake = 4096                                                  # never dereferenced: every case below is refused by the argument checks

    def call(N=8, E=16, off=(0, 10, 20), T=None, img=fake, prm=fake, logits=fake, ld=None, row=0):
        C = len(off) - 1
        arr = (ctypes.c_int32 * len(off))(*off)
        return lib.uia_zero_shot_score(None, N, off[-1] if T is None else T, E, C, arr, img, prm, logits, C if ld is None else ld, row, None, None)

    for kw, text in ((dict(off=(0, 5)), b"C=1"), (dict(off=tuple(range(10))), b"C=9"), (dict(off=(0, 33, 40)), b"33 prompts"), (dict(off=(0, 0, 4)), b"0 prompts"),
                     (dict(off=tuple(32 * c for c in range(8)) + (257,)), b"T=257"), (dict(T=0), b"T=0"), (dict(E=0), b"E=0"), (dict(E=4097), b"E=4097"),
                     (dict(N=0), b"N=0"), (dict(N=(1 << 24) + 1), b"N="), (dict(off=(1, 10, 20)), b"class_off"), (dict(T=21), b"class_off"),
                     (dict(off=(0, 12, 8, 20)), b"prompts"), (dict(img=None), b"null"), (dict(prm=None), b"null"), (dict(logits=None), b"null"),
                     (dict(ld=1), b"leading"), (dict(row=-1), b"row")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_zero_shot_score" in msg and text in msg, (kw, msg)


def test_roc_argument_checks_and_workspace():
    from uia_hip import _lib
    lib = _lib.lib()
    assert lib.uia_binary_roc_curve_workspace_bytes(0) == 0 and lib.uia_binary_roc_curve_workspace_bytes(1000) == 5000
    fake = 4096

    def call(N=100, p1=fake, labels=fake, perm=fake, ws=fake, ws_bytes=500, count=fake, fpr=fake, tpr=fake, thr=fake):
        return lib.uia_binary_roc_curve(None, N, p1, labels, perm, ws, ws_bytes, count, fpr, tpr, thr)

    for kw, text in ((dict(N=0), b"N=0"), (dict(N=(1 << 24) + 1), b"N="), (dict(p1=None), b"null"), (dict(labels=None), b"null"), (dict(perm=None), b"null"),
                     (dict(ws=None), b"null"), (dict(count=None), b"null"), (dict(fpr=None), b"null"), (dict(tpr=None), b"null"), (dict(thr=None), b"null"),
                     (dict(ws_bytes=499), b"workspace")):
        assert call(**kw) != 0, kw
        msg = lib.uia_last_error()
        assert b"uia_binary_roc_curve" in msg and text in msg, (kw, msg)


def test_ops_refuse_cpu_tensors():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    with pytest.raises(UiaError):
        ops.zero_shot_score(torch.randn(4, 16), torch.randn(20, 16), [0, 10, 20])
    with pytest.raises(UiaError):
        ops.binary_roc_curve(torch.rand(8), torch.randint(0, 2, (8,)))


# ------------------------------------------------------------------------------------------------ host helpers of the loop
def test_collapse_ratio_and_prototype_similarity():
    from src.models import zero_shot_eval as ZS
    g = torch.Generator().manual_seed(0)
    d = torch.nn.functional.normalize(torch.randn(1, 32, generator=g), dim=1)
    assert ZS.collapse_ratio(d.repeat(10, 1)) is None                        # the reference needs more than ten rows
    assert ZS.collapse_ratio(d.repeat(40, 1)) > 0.999
    spread = torch.nn.functional.normalize(torch.randn(400, 32, generator=g), dim=1)
    assert ZS.collapse_ratio(spread) < 0.2
    prm = torch.cat([d.repeat(3, 1) * 4.0, -d.repeat(2, 1)])
    assert abs(ZS.prototype_similarity(prm, [0, 3, 5]) + 1.0) < 1e-6
    assert abs(ZS.prototype_similarity(torch.cat([d, 2 * d]), [0, 1, 2]) - 1.0) < 1e-6


def test_report_writes_the_folder_without_a_checkpoint(tmp_path):
    import argparse
    import logging
    from src.models import zero_shot_eval as ZS
    from src.utils.tools import setup_logging
    args = argparse.Namespace(test_snapshot_path=str(tmp_path / "t"))
    setup_logging(args, args.test_snapshot_path)
    stats = dict(acc=0.625, rec=0.5, pre=1.0, f1=2 / 3, auc=0.7, loss=0.1, n=8)
    folder = ZS.report(args, "clip", stats, ([0.0, 0.25, 1.0], [0.0, 1 / 3, 1.0], [1.0, 0.75, 0.5]))
    logging.shutdown()
    assert os.path.basename(folder).endswith("_acc=62.50") and sorted(os.listdir(folder))[:2] == ["log.log", "results.csv"]
    assert open(os.path.join(folder, "results.csv")).read() == "Metric,Mean\nAcc,62.50\nRec,50.00\nPre,100.00\nF1,66.67\nAUC,70.00\n"
    assert open(os.path.join(folder, "roc_curve.csv")).read() == "fpr,tpr,threshold\n0.0,0.0,1.0\n0.25,0.3333333333333333,0.75\n1.0,1.0,0.5\n"
    assert "CLIP Zero-shot Results" in open(os.path.join(folder, "log.log")).read()
    assert not os.path.exists(os.path.join(folder, "best_model.pth"))


if __name__ == "__main__":                                                   # records the reference's tables: python tests/test_zero_shot_host.py <reference src/models>
    tables = {e: _argparse_table(os.path.join(sys.argv[1], e)) for e in ENTRIES}
    with open(GOLDEN_TABLES, "w") as f:
        json.dump(tables, f, indent=1, sort_keys=True)
        f.write("\n")
