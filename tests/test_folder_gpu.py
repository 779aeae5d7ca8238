"""-m gpu: the --data_root path end to end on a 12-picture tree (tests/folder_tree.py).  The folder loader's validation batches, through
RaggedPrefetcher and ResizeStage (one uia_resize_batch launch each), equal bit for bit the batches of a --data_pt file that PIL made from the same
files on the host — segmentation (images and masks) and classification (images and labels); and the two baseline entries train, validate and test
from the folders, with the augmentation stage acting on their batches."""
import csv
import glob
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytest.importorskip("PIL")
import folder_tree as T  # noqa: E402

S = 32


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return T.write_tree(tmp_path_factory.mktemp("data"))


def _args(**kw):
    a = dict(data_root=None, data_pt=None, synthetic=False, dataset=T.DATASET, img_size=S, batch_size=2, num_workers=0, seed=3, device="cuda:0")
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("kind", ["segmentation", "classification"])
def test_resize_stage_gives_the_data_pt_batch_bit_for_bit(tree, tmp_path, kind):
    from src.datasets import folder as F
    from src.models import supervised as L
    from uia_hip.engine import DevicePrefetcher
    task = L.SEGMENTATION if kind == "segmentation" else L.CLASSIFICATION
    pt = T.write_data_pt(tree, tmp_path / "data.pt", S, kind)
    want = []
    pf = DevicePrefetcher(task.data.DataModule(_args(data_pt=pt), rank=0, world=1).val_dataloader(), None, "cuda:0", second=task.data.second_of)
    for images, second, ready in pf:
        torch.cuda.current_stream().wait_event(ready)
        want.append((images.cpu(), second.cpu()))
    pf.close()
    stage = F.stage_for(_args(data_root=tree), task.with_mask)
    got = []
    pf = F.RaggedPrefetcher(F.DataModule(_args(data_root=tree), kind).val_dataloader(), "cuda:0")
    for batch, second, ready in pf:
        torch.cuda.current_stream().wait_event(ready)
        images, second = stage(batch, second)
        got.append((images.cpu(), second.cpu()))
    pf.close()
    assert [tuple(i.shape) for i, _ in got] == [(2, 1, S, S), (1, 1, S, S)] == [tuple(i.shape) for i, _ in want]      # three pictures: a ragged last batch
    for (gi, gs), (wi, ws) in zip(got, want):
        assert gi.dtype == wi.dtype == torch.float32 and torch.equal(gi.view(torch.int32), wi.view(torch.int32))
        assert gs.dtype == ws.dtype and torch.equal(gs, ws)
    if kind == "segmentation":
        assert any(bool(s.any()) and not bool(s.all()) for _, s in got)


@pytest.mark.parametrize("entry, exp, keys", [("segmentation", "unet_seg", ("Dice", "IoU", "HD95", "ASD")),
                                              ("classification", "resnet_cls", ("Acc", "Rec", "Pre", "F1", "AUC"))])
def test_baseline_entry_trains_validates_and_tests_from_the_folders(tree, tmp_path, entry, exp, keys):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))
    stats = tmp_path / "stats.json"
    cmd = [sys.executable, "-m", f"src.models.baselines.{entry}", "--data_root", tree, "--dataset", T.DATASET, "--img_size", str(S), "--epochs", "2",
           "--batch_size", "4", "--num_workers", "2", "--val_every", "1", "--stats_json", str(stats)]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.load(open(stats))
    assert out["iters"] == 2 and out["augmented_images"] > 0, out                                 # six training pictures, drop_last: one batch per epoch
    run = tmp_path / "runs" / exp / T.DATASET
    assert (run / "train" / "best_model.pth").exists() and (run / "train" / "log" / "scalars.jsonl").exists()
    found = glob.glob(str(run / "test" / "**" / "results.csv"), recursive=True)
    assert found
    rows = {row[0]: row[1:] for row in csv.reader(open(found[0]))}
    for key in keys:
        assert key in rows and rows[key][0] != "" and np.isfinite(float(rows[key][0])), rows
    if entry == "segmentation":
        pictures = {os.path.basename(p) for p in glob.glob(str(run / "test" / "**" / "*.png"), recursive=True)}
        assert {n for n in T.SPLITS["test"]} <= pictures, pictures                                  # the visualiser names its pictures by name_of(i)
