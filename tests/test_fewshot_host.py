"""Host checks of the few-shot path: the sampler against name lists recorded from the reference's own _sample_training_data
(tests/golden/fewshot_samples.json, written by tools/gen_fewshot_golden.py), the four CLIs against the reference's argparse tables, the refusals, the
resident set's batch contract with a stubbed launch, and the new export."""
import ast
import ctypes
import json
import os
import random
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

ENTRIES = ["biomedclip/fewshot_classification.py", "biomedclip/fewshot_segmentation.py", "baselines/fewshot_classification.py",
           "baselines/fewshot_segmentation.py"]
ADDITIONS = ["--dtype", "--synthetic", "--synthetic_train", "--synthetic_val", "--synthetic_test", "--data_pt", "--ckpt_path", "--model_config",
             "--extract_layers", "--val_every", "--stats_json"]


def _samples():
    return json.load(open(os.path.join(HERE, "golden", "fewshot_samples.json")))


# ------------------------------------------------------------------------------------------------ the sampler
def test_fixture_covers_the_recorded_strategies():
    z = _samples()
    small = z["sets"]["small"]
    assert len(small["names"]) >= 40 and sorted((small["labels"].count(0), small["labels"].count(1))) == [16, 24]
    cls = [c for c in z["cases"] if c["task"] == "classification"]
    seg = [c for c in z["cases"] if c["task"] == "segmentation"]
    assert {c["seed"] for c in z["cases"]} == {1, 2}
    assert {c["train_ratio"] for c in seg} == {0.01, 0.1, 1.0}
    assert {c["shots_per_class"] for c in cls if "shots_per_class" in c} == {1, 2, 100}
    assert {(c["train_ratio"], c["stratified"]) for c in cls if "shots_per_class" not in c} == {(r, s) for r in (0.01, 0.1, 1.0) for s in (True, False)}


def test_sampler_reproduces_every_recorded_list_and_leaves_the_global_generator_alone():
    from src.datasets import fewshot_classification as C
    from src.datasets import fewshot_segmentation as S
    z = _samples()
    random.seed(1234)
    before = random.getstate()
    for c in z["cases"]:
        names, labels = z["sets"][c["set"]]["names"], z["sets"][c["set"]]["labels"]
        rng = random.Random(c["seed"])
        if c["task"] == "segmentation":
            got = S.sample_training_names(list(names), c["train_ratio"], rng)
        else:
            got = C.sample_training_names(list(names), dict(zip(names, labels)), c.get("train_ratio"), c.get("shots_per_class"), c.get("stratified", True), rng)
        assert got == c["sampled"], {k: v for k, v in c.items() if k != "sampled"}
    assert random.getstate() == before
    # the strategies' shapes: the stratified ratio 1.0 is a permutation, not the identity; the segmentation ratio 1.0 is the list itself
    names = z["sets"]["small"]["names"]
    one = [c for c in z["cases"] if c["set"] == "small" and c.get("train_ratio") == 1.0 and "shots_per_class" not in c]
    for c in one:
        assert sorted(c["sampled"]) == sorted(names)
        assert (c["sampled"] == names) == (c["task"] == "segmentation")


def _args(**kw):
    a = dict(data_pt=None, synthetic=True, synthetic_train=40, synthetic_val=6, synthetic_test=8, img_size=16, seed=1, batch_size=4, num_workers=0,
             train_ratio=0.1, shots_per_class=None)
    a.update(kw)
    return SimpleNamespace(**a)


def test_data_modules_sample_the_training_split_only_and_print_the_reference_lines(capsys, tmp_path):
    from src.datasets import classification as DC
    from src.datasets import fewshot_classification as C
    from src.datasets import fewshot_segmentation as S
    random.seed(99)
    before = random.getstate()
    dm = C.from_args(_args(shots_per_class=3))
    out = capsys.readouterr().out
    assert "  Few-shot sampling:\n    - Original training samples: 40\n    - Sampled training samples: 6\n    - Shots per class: 3\n" in out
    assert (dm.original_train_count, dm.sampled_train_count) == (40, 6) and len(dm.val_dataset) == 6 and len(dm.test_dataset) == 8
    full = DC.DataModule(_args())
    want = C.sample_training_names(list(full.train_dataset.names), dict(zip(full.train_dataset.names, full.train_dataset.labels.tolist())), None, 3, True,
                                   random.Random(1))
    assert dm.train_dataset.names == want
    images, labels = dm.resident_rows()
    assert images.shape == (6, 1, 16, 16) and images.dtype == torch.float32 and labels.dtype == torch.int64 and sorted(labels.tolist()) == [0, 0, 0, 1, 1, 1]
    for k, name in enumerate(want):
        i = full.train_dataset.names.index(name)
        assert torch.equal(images[k], full.train_dataset.images[i]) and int(labels[k]) == int(full.train_dataset.labels[i])

    dm = S.from_args(_args(train_ratio=0.1))
    out = capsys.readouterr().out
    assert "    - Sampled training samples: 4\n    - Train ratio: 10.0%\n" in out
    images, masks = dm.resident_rows()
    assert images.shape == masks.shape == (4, 1, 16, 16) and masks.dtype == torch.uint8 and len(dm.test_dataset) == 8
    whole = S.from_args(_args(train_ratio=1.0))
    assert whole.sampled_train_count == 40 and [whole.train_dataset.name_of(i) for i in range(40)] == [f"train_{i:05d}.png" for i in range(40)]

    # a uint8 --data_pt file stays uint8 (channel 0), masks become {0, 1} bytes
    g = torch.Generator().manual_seed(0)
    blob = {"images": torch.randint(0, 256, (20, 3, 16, 16), generator=g, dtype=torch.uint8), "labels": torch.randint(0, 2, (20, 1, 16, 16), generator=g, dtype=torch.uint8) * 255}
    torch.save(blob, tmp_path / "seg.pt")
    dm = S.from_args(_args(data_pt=str(tmp_path / "seg.pt"), train_ratio=0.2))
    images, masks = dm.resident_rows()
    assert images.dtype == torch.uint8 and images.shape == (2, 1, 16, 16) and set(masks.unique().tolist()) <= {0, 1}
    idx = [int(n[:5]) for n in dm.train_dataset.names]
    assert torch.equal(images, blob["images"][idx][:, :1]) and torch.equal(masks, (blob["labels"][idx] > 0).to(torch.uint8))
    assert random.getstate() == before


# ------------------------------------------------------------------------------------------------ CLI tables
@pytest.mark.parametrize("entry", ENTRIES)
def test_fewshot_cli_carries_every_reference_flag_and_default(entry):
    import importlib
    from oracle.gen_host_fixtures import argparse_table
    ref = json.load(open(os.path.join(HERE, "golden", "reference_fewshot_cli_tables.json")))[entry]
    assert len(ref) >= 20 and "--train_ratio" in ref and ("--shots_per_class" in ref) == entry.endswith("classification.py")
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
    assert args["exp"].startswith("fewshot_") and args["val_every"] == 10
    base = importlib.import_module("src.models." + entry[:-3].replace("/", ".").replace("fewshot_", ""))
    assert mod.prepare_model is base.prepare_model


def test_fewshot_tasks_are_the_supervised_ones_with_three_fields_set():
    import dataclasses
    from src.models import supervised as L
    for task, base in ((L.FEWSHOT_CLASSIFICATION, L.CLASSIFICATION), (L.FEWSHOT_SEGMENTATION, L.SEGMENTATION)):
        assert task.resident and task.train_module is not None and not task.data_parallel and task.data is base.data and task.criterion is base.criterion
        assert not base.resident and base.train_module is None and not base.roc_csv
        changed = {f.name for f in dataclasses.fields(L.Task) if getattr(task, f.name) != getattr(base, f.name)}
        assert changed <= {"train_module", "resident", "roc_csv", "data_parallel"}
    assert L.FEWSHOT_CLASSIFICATION.roc_csv and not L.FEWSHOT_SEGMENTATION.roc_csv


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_ratio_bad_shots_and_more_than_one_process_are_refused(entry, monkeypatch):
    import importlib
    mod = importlib.import_module("src.models." + entry[:-3].replace("/", "."))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mod.check_args(mod.get_args(["--train_ratio", "1.0"]))
    for bad in ("0", "-0.1", "1.01"):
        with pytest.raises(ValueError, match="train_ratio"):
            mod.check_args(mod.get_args(["--train_ratio", bad]))
        with pytest.raises(ValueError, match="train_ratio"):
            mod.main(["--train_ratio", bad, "--synthetic"])                      # main refuses before anything is allocated
    if entry.endswith("classification.py"):
        for bad in ("0", "-2"):
            with pytest.raises(ValueError, match="shots_per_class"):
                mod.check_args(mod.get_args(["--shots_per_class", bad]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process"):
        mod.check_args(mod.get_args([]))
    with pytest.raises(ValueError, match="one process"):
        mod.train(mod.get_args(["--synthetic"]))
    from src.models import supervised
    with pytest.raises(ValueError, match="one process"):
        supervised.train(mod.get_args(["--synthetic"]), mod.TASK, mod.prepare_model)      # the loop itself, past the entry's own check


def test_data_module_refuses_a_world_above_one():
    from src.datasets import fewshot_segmentation as S
    with pytest.raises(ValueError, match="one process"):
        S.FewShotDataModule(_args(), train_ratio=0.1, rank=0, world=2)


# ------------------------------------------------------------------------------------------------ the batch contract
@pytest.mark.parametrize("n", [1, 5, 32, 33, 70])
@pytest.mark.parametrize("with_mask", [False, True])
def test_resident_batches_follow_the_reference_loader_contract(n, with_mask):
    """B = min(32, n), drop_last = n > 32, a fresh permutation per epoch: every batch has B rows, an epoch has n // B batches, no row twice in an epoch, all of
    them when n <= 32.  The launch is a stub that reads the table's src column as the kernel would."""
    from src.datasets import resident as R
    S = 8
    images = (torch.arange(n, dtype=torch.float32)[:, None, None, None] + torch.zeros(n, 1, S, S)).contiguous()
    second = (torch.arange(n, dtype=torch.uint8)[:, None, None, None] + torch.zeros(n, 1, S, S, dtype=torch.uint8)) if with_mask else torch.arange(n) * 10
    calls = []

    def launch(res_images, res_masks, table, out_images, out_masks, ws):
        t = table.numpy()
        assert t.shape == (min(32, n), 14, 4) and (t[:, 0, 0] == 0).all() and (t[:, 0, 1] == int(with_mask)).all()
        src = torch.from_numpy(t[:, 0, 2].astype(np.int64))
        out_images.copy_(res_images[src])
        if with_mask:
            out_masks.copy_(res_masks[src])
        calls.append(src.tolist())

    rs = R.ResidentTrainSet(images, second, 32, seed=3, device="cpu", launch=launch)
    B, iters = min(32, n), (n // 32 if n > 32 else 1)
    assert (rs.B, len(rs)) == (B, iters) == R.batch_plan(n, 32)
    epochs = []
    for epoch in range(3):
        rs.set_epoch(epoch)
        seen = []
        for im, lab, ready in rs:
            rows = im[:, 0, 0, 0].long().tolist()
            assert len(rows) == B and rows == calls[-1]
            assert (lab[:, 0, 0, 0].long().tolist() == rows) if with_mask else (lab.tolist() == [10 * r for r in rows])
            seen += rows
        assert len(seen) == iters * B and len(set(seen)) == len(seen) and set(seen) <= set(range(n))
        if n <= 32:
            assert sorted(seen) == list(range(n))
        epochs.append(seen)
    assert len(calls) == 3 * iters and rs.augmented == 0
    if n >= 5:
        assert epochs[0] != epochs[1] or epochs[1] != epochs[2]                     # a fresh permutation per epoch
    rs.set_epoch(0)
    assert [r for im, _, _ in rs for r in im[:, 0, 0, 0].long().tolist()] == epochs[0]      # ... a function of (seed, epoch)


def test_resident_programs_are_the_stage_draws_with_the_src_column_added():
    from src.datasets import augment as A
    from src.datasets import resident as R
    n, S = 6, 16
    tables = []
    rs = R.ResidentTrainSet(torch.zeros(n, 1, S, S, dtype=torch.uint8), torch.zeros(n, 1, S, S, dtype=torch.uint8), 4, strong=True, weak=True, seed=5, rank=0,
                            device="cpu", launch=lambda *a: tables.append(a[2].numpy().copy()))
    rs.set_epoch(2)
    list(rs)
    assert len(tables) == 1
    want = A.draw_programs(4, S, True, True, True, A.make_rng(5, 0, 2, 0))
    perm = R.epoch_permutation(n, 5, 2)
    assert np.array_equal(tables[0][:, 0, 2], perm[:4])
    got = tables[0].copy()
    got[:, 0, 2] = 0
    assert np.array_equal(got, want) and rs.augmented == int((want[:, 0, 0] > 0).sum())
    with pytest.raises(ValueError):
        R.ResidentTrainSet(torch.zeros(2, 1, 16, 12), torch.zeros(2, dtype=torch.int64), 4, device="cpu", launch=lambda *a: None)


# ------------------------------------------------------------------------------------------------ the export
def test_augment_gather_is_exported_and_declared():
    from uia_hip import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(handle, "uia_augment_gather") and "uia_augment_gather" in _lib.PROTOTYPES
    assert "uia_augment_gather" in open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    assert "uia_augment_gather" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_augment_gather_host_checks_run_before_anything_is_enqueued():
    """No device here: every refusal below returns non-zero from the host checks with the outputs untouched (host memory stands in for the tensors)."""
    from uia_hip import _lib
    lib = _lib.lib()
    N, B, S = 5, 7, 9
    img = np.zeros((N, 1, S, S), np.uint8)
    msk = np.zeros((N, 1, S, S), np.uint8)
    out = np.full((B, 1, S, S), 7.0, np.float32)
    outm = np.full((B, 1, S, S), 0xA5, np.uint8)
    need = lib.uia_augment_workspace_bytes(B, S)
    assert need == lib.uia_augment_workspace_bytes(B, S) > 0
    ws = np.zeros(need + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    good = np.zeros((B, 14, 4), np.int32)
    good[:, 0, 1], good[:, 0, 2] = 1, [0, 4, 4, 2, 1, 0, 3]

    def call(tab=good, N=N, B=B, dt=1, images=img.ctypes.data, masks=msk.ctypes.data, out_images=out.ctypes.data, out_masks=outm.ctypes.data):
        tab = np.ascontiguousarray(tab, dtype=np.int32)
        return lib.uia_augment_gather(None, N, B, S, dt, images, masks, tab.ctypes.data, wsp, need, out_images, out_masks), lib.uia_last_error().decode()

    def with_src(v):
        t = good.copy()
        t[3, 0, 2] = v
        return t

    for what, kw, word in [("src = N", dict(tab=with_src(N)), "row"), ("src = -1", dict(tab=with_src(-1)), "row"), ("src_dtype = 2", dict(dt=2), "src_dtype"),
                           ("N = 0", dict(N=0), "N"), ("output inside the resident images", dict(out_images=img.ctypes.data + 4 * S * S), "overlap"),
                           ("mask output inside the resident masks", dict(out_masks=msk.ctypes.data + (N - 1) * S * S), "overlap"),
                           ("masks without an output", dict(out_masks=None), "go together")]:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_augment_gather" in err, (what, rc, err)
    assert (out == 7.0).all() and (outm == 0xA5).all()
