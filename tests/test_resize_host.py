"""Host checks of the --data_root path: the plain-Python restatement of Pillow's resize (src/datasets/pil_resize.py) against the recorded fixture
(tests/golden/resize_pil.npz, tools/gen_resize_golden.py) and, where Pillow is installed, against live Image.resize; the argument checks of
uia_resize_batch, which all fail before any GPU call; and the folder loader (src/datasets/folder.py) on a tree written into tmp_path."""
import ctypes
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

import folder_tree as T  # noqa: E402
import resize_cases as RC  # noqa: E402

# W x H -> S: the square squashes the restatement was first checked on
LIVE = [(471, 562, 224), (224, 300, 224), (100, 90, 224), (1024, 768, 224), (333, 517, 518), (37, 1023, 32), (224, 224, 224), (225, 223, 224),
        (600, 448, 224), (9, 8, 16)]


# ------------------------------------------------------------------------------------------------ the restatement
def test_fixture_covers_every_path():
    expected, version = RC.load_golden()
    assert version and len(expected) == len(RC.CASES) == 16
    from src.datasets.pil_resize import ksize_of
    assert max(ksize_of(c["H"], c["dst_h"]) for c in RC.CASES) == 129
    assert any(c["W"] < c["dst_w"] and c["H"] < c["dst_h"] for c in RC.CASES)                       # an upscale
    assert any((c["W"] == c["dst_w"]) != (c["H"] == c["dst_h"]) for c in RC.CASES)                   # one pass skipped
    assert any(c["W"] == c["dst_w"] and c["H"] == c["dst_h"] for c in RC.CASES)                      # both
    assert any(c["C"] == 3 and (c["x0"] or c["y0"]) for c in RC.CASES)
    for cases in RC.LISTS.values():
        assert any(c["kind"] == "smooth" for c in cases)
        smooth = [expected[c["name"]][0] for c in cases if c["kind"] == "smooth"]
        assert any((s == 0).any() and (s == 255).any() for s in smooth)                            # clip8 clips on both sides


@pytest.mark.parametrize("case", RC.CASES, ids=[c["name"] for c in RC.CASES])
def test_restatement_equals_the_fixture_in_every_byte(case):
    from src.datasets import pil_resize as R
    want_i, want_m = RC.load_golden()[0][case["name"]]
    px, mask = RC.make_input(case)
    got = R.resize_bicubic(px, case["dst_h"], case["dst_w"], RC.window_of(case))
    assert got.shape == want_i.shape and int((got != want_i).sum()) == 0
    if mask is not None:
        got_m = (R.resize_nearest(mask, case["dst_h"], case["dst_w"], RC.window_of(case)) != 0).astype(np.uint8)
        assert int((got_m != want_m).sum()) == 0


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    from src.datasets import pil_resize as R
    for W, H, S in LIVE:
        rng = np.random.default_rng(W * 1000 + H)
        px = rng.integers(0, 256, (H, W), dtype=np.uint8)
        want = np.asarray(Image.fromarray(px, "L").resize((S, S)))
        assert int((R.resize_bicubic(px, S, S) != want).sum()) == 0, (W, H, S)
        mask = Image.fromarray(rng.integers(0, 2, (H, W), dtype=np.uint8) * 255, "L").convert("1")
        want_m = np.asarray(mask.resize((S, S)), dtype=np.uint8)
        got_m = (R.resize_nearest(np.asarray(mask).view(np.uint8), S, S) != 0).astype(np.uint8)
        assert int((got_m != want_m).sum()) == 0, (W, H, S)
    px = np.random.default_rng(5).integers(0, 256, (451, 300, 3), dtype=np.uint8)                   # RGB 300 x 451 -> 224 x 336, and its centre window
    want = np.asarray(Image.fromarray(px, "RGB").resize((224, 336), Image.BICUBIC))
    assert int((R.resize_bicubic(px, 336, 224) != want).sum()) == 0
    assert int((R.resize_bicubic(px, 336, 224, (56, 0, 224, 224)) != want[56:280]).sum()) == 0


# ------------------------------------------------------------------------------------------------ the C entry
def test_resize_batch_is_exported_and_declared():
    from uia_hip import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uia_resize_batch", "uia_resize_workspace_bytes"):
        assert hasattr(handle, name) and name in _lib.PROTOTYPES
        assert name in open(os.path.join(ROOT, "include", "uia_hip.h")).read()
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_resize_batch_host_checks_run_before_anything_is_enqueued():
    """No device here: every refusal returns non-zero from the host checks with the outputs untouched (host memory stands in for the tensors)."""
    from uia_hip import _lib
    lib = _lib.lib()
    B, S = 3, 16
    src = np.zeros(4096, np.uint8)
    out = np.full((B, 3, S, S), 7.0, np.float32)
    outm = np.full((B, 1, S, S), 0xA5, np.uint8)
    assert lib.uia_resize_workspace_bytes(0) == 0 and lib.uia_resize_workspace_bytes(65536) == 0
    need = lib.uia_resize_workspace_bytes(B)
    assert need >= B * 32
    ws = np.zeros(need + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    good = np.array([[0, 20, 30, 600, S, S, 0, 0], [1200, 9, 8, -1, S, S, 0, 0], [1300, 16, 16, 1600, 24, 20, 8, 4]], np.int32)

    def call(desc=good, B=B, C=1, S=S, src_p=src.ctypes.data, n=src.size, out_images=out.ctypes.data, out_masks=outm.ctypes.data, ws_bytes=need):
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        return lib.uia_resize_batch(None, B, C, S, src_p, n, desc.ctypes.data, wsp, ws_bytes, out_images, out_masks), lib.uia_last_error().decode()

    def with_(b, col, v):
        d = good.copy()
        d[b, col] = v
        return d

    refusals = [("B = 0", dict(B=0), "B=0"), ("B = 65536", dict(B=65536), "B=65536"), ("S = 7", dict(S=7), "S=7"), ("S = 1025", dict(S=1025), "S=1025"),
                ("C = 2", dict(C=2), "C=2"), ("H = 0", dict(desc=with_(1, 1, 0)), "image 1"), ("W = 0", dict(desc=with_(2, 2, 0)), "image 2"),
                ("image leaves the buffer", dict(desc=with_(1, 0, 4096 - 71)), "image 1"), ("negative offset", dict(desc=with_(0, 0, -4)), "image 0"),
                ("mask leaves the buffer", dict(desc=with_(2, 3, 4096 - 255)), "image 2"), ("mask offset -2", dict(desc=with_(0, 3, -2)), "image 0"),
                ("window leaves dst, rows", dict(desc=with_(2, 6, 9)), "image 2"), ("window leaves dst, columns", dict(desc=with_(2, 7, 5)), "image 2"),
                ("negative corner", dict(desc=with_(2, 6, -1)), "image 2"), ("dst smaller than the window", dict(desc=with_(0, 4, S - 1)), "image 0"),
                ("dst = 0", dict(desc=with_(0, 5, 0)), "image 0"),
                ("a 33x downscale", dict(desc=np.array([[0, 16, 16, -1, S, S, 0, 0], [0, 33 * S, 1, -1, S, S, 0, 0]], np.int32), B=2), "image 1"),
                ("a mask without out_masks", dict(out_masks=None), "image 0"), ("a short workspace", dict(ws_bytes=need - 1), "workspace"),
                ("null source", dict(src_p=None), "null"), ("output inside the source", dict(out_images=src.ctypes.data + 64), "overlap"),
                ("mask output inside the source", dict(out_masks=src.ctypes.data + 2048), "overlap")]
    for what, kw, word in refusals:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_resize_batch" in err, (what, rc, err)
    assert (out == 7.0).all() and (outm == 0xA5).all()


# ------------------------------------------------------------------------------------------------ the folder loader
def _args(root, **kw):
    a = dict(data_root=None if root is None else str(root), data_pt=None, synthetic=False, dataset=T.DATASET, img_size=32, batch_size=4, num_workers=0, seed=3)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL")
    return T.write_tree(tmp_path_factory.mktemp("data"))


def test_folder_splits_labels_and_names(tree):
    from PIL import Image
    from src.datasets import folder as F
    for kind in ("segmentation", "classification"):
        dm = F.DataModule(_args(tree), kind)
        for split, ds in (("train", dm.train_dataset), ("val", dm.val_dataset), ("test", dm.test_dataset)):
            assert ds.names == T.SPLITS[split] and [ds.name_of(i) for i in range(len(ds))] == T.SPLITS[split]
            assert ds.sizes == [T.size_of(T.NAMES.index(n)) for n in ds.names]
        px, second, name = dm.val_dataset[1]
        W, H = T.size_of(7)
        assert name == "img_07.png" and px.dtype == np.uint8 and px.shape == (H, W)
        assert np.array_equal(px, np.asarray(Image.open(os.path.join(tree, "all/images", name)).convert("L")))      # the luma of an RGB file, not its red channel
        assert not np.array_equal(px, np.asarray(Image.open(os.path.join(tree, "all/images", name)))[..., 0])
        if kind == "classification":
            assert second == T.LABELS[name] and dm.train_dataset.labels == [T.LABELS[n] for n in T.SPLITS["train"]]
        else:
            assert second.dtype == np.uint8 and second.shape == (H, W) and set(np.unique(second != 0).tolist()) == {False, True}


def test_ragged_collate_packs_bytes_descriptor_labels_and_names(tree):
    from src.datasets import folder as F
    for kind in ("segmentation", "classification"):
        dm = F.DataModule(_args(tree), kind)
        batches = list(dm.val_dataloader()) + list(dm.test_dataloader())
        assert [b[3] for b in batches] == [T.SPLITS["val"], T.SPLITS["test"]]                      # whole, in file order
        buf, desc, labels, names = batches[0]
        assert buf.dtype == torch.uint8 and buf.dim() == 1 and desc.dtype == torch.int32 and tuple(desc.shape) == (3, F.DESC)
        at = 0
        for b, n in enumerate(names):
            px, second, _ = dm.val_dataset[b]
            H, W = px.shape
            off, h, w, moff, dh, dw, y0, x0 = desc[b].tolist()
            assert (off, h, w, dh, dw, y0, x0) == (at, H, W, 32, 32, 0, 0)
            assert np.array_equal(buf[off:off + H * W].numpy().reshape(H, W), px)
            at += H * W
            if kind == "segmentation":
                assert moff == at and np.array_equal(buf[moff:moff + H * W].numpy().reshape(H, W), second)
                at += H * W
            else:
                assert moff == -1
        assert buf.numel() == at
        assert labels is None if kind == "segmentation" else labels.tolist() == [T.LABELS[n] for n in names]
        train = list(dm.train_dataloader())
        assert len(train) == 1 and len(train[0][3]) == 4 and set(train[0][3]) <= set(T.SPLITS["train"])      # shuffled, drop_last


def test_training_split_is_sharded_by_rank(tree):
    from src.datasets import folder as F
    seen = []
    for rank in range(2):
        dm = F.DataModule(_args(tree, batch_size=3), "segmentation", rank=rank, world=2)
        loader = dm.train_dataloader()
        dm.set_epoch(0)
        first = [n for b in loader for n in b[3]]
        assert len(first) == 3 and len(loader) == 1
        seen.append(set(first))
        assert [b[3] for b in dm.val_dataloader()] == [T.SPLITS["val"]]                            # validation runs whole on every rank
    assert not (seen[0] & seen[1]) and seen[0] | seen[1] == set(T.SPLITS["train"])


def test_precedence_data_pt_then_synthetic_then_data_root(tree, tmp_path):
    from src.datasets import folder as F
    from src.datasets.augment import stage_for
    from src.models import supervised as L
    assert F.chosen(_args(tree)) and not F.chosen(_args(tree, synthetic=True)) and not F.chosen(_args(tree, data_pt="x.pt")) and not F.chosen(_args(None))
    syn = dict(synthetic=True, synthetic_train=8, synthetic_val=4, synthetic_test=4)
    assert isinstance(L._data_module(_args(tree), L.SEGMENTATION, 0, 1), F.DataModule)
    assert isinstance(L._data_module(_args(tree), L.CLASSIFICATION, 0, 1), F.DataModule)
    assert isinstance(L._data_module(_args(tree, **syn), L.CLASSIFICATION, 0, 1), L.CLASSIFICATION.data.DataModule)
    pt = T.write_data_pt(tree, tmp_path / "cls.pt", 32, "classification")
    dm = L._data_module(_args(tree, data_pt=pt, **syn), L.CLASSIFICATION, 0, 1)
    assert isinstance(dm, L.CLASSIFICATION.data.DataModule) and dm.val_dataset.names == T.SPLITS["val"]
    with pytest.raises(RuntimeError, match="no dataset"):                                         # none of the three: as before
        L._data_module(_args(None), L.SEGMENTATION, 0, 1)
    assert F.stage_for(_args(tree), True) is not None and F.stage_for(_args(tree, synthetic=True), True) is None
    on = dict(strong_augs=True, weak_augs=True)
    assert stage_for(_args(tree, **on), with_mask=True) is not None and stage_for(_args(tree, synthetic=True, **on), with_mask=True) is None
    assert stage_for(_args(tree, strong_augs=False, weak_augs=False), with_mask=True) is None
    p = __import__("argparse").ArgumentParser()
    L.add_build_args(p)
    assert p.parse_args([]).data_root is None and p.parse_args(["--data_root", "d"]).data_root == "d"


def test_a_file_outside_the_kernels_limits_is_refused_by_name(tree, tmp_path):
    import shutil
    from PIL import Image
    from src.datasets import folder as F
    root = str(tmp_path / "copy")
    shutil.copytree(tree, root)
    Image.fromarray(np.zeros((33 * 32, 8), np.uint8), "L").save(os.path.join(root, "all/images", "img_10.png"))       # 33x taller than --img_size 32
    with pytest.raises(RuntimeError, match=r"img_10\.png.*129"):
        F.DataModule(_args(root), "classification")
    with pytest.raises(RuntimeError, match=r"mask of img_10\.png"):                              # and its mask no longer has its size
        F.DataModule(_args(root), "segmentation")
    with pytest.raises(RuntimeError, match="img_size"):
        F.DataModule(_args(tree, img_size=2048), "classification")


def test_entries_outside_the_scope_refuse_data_root(tree):
    from src.datasets import folder as F
    from src.models import contrastive, supervised as L, zero_shot_eval
    from src.models.biomedclip import retrieval
    from src.models.clipseg import segmentation as clipseg
    for task in (L.FEWSHOT_CLASSIFICATION, L.FEWSHOT_SEGMENTATION):
        with pytest.raises(RuntimeError, match="few-shot"):
            L.run(_args(tree, exp="x", test=False), task, None)
    with pytest.raises(RuntimeError, match="CLIPSeg"):
        clipseg.check_args(_args(tree, dataset="BUSI"))
    with pytest.raises(RuntimeError, match="contrastive"):
        contrastive.run(_args(tree), None, None, None)
    with pytest.raises(RuntimeError, match="zero-shot"):
        zero_shot_eval.load_test_split(_args(tree))
    with pytest.raises(RuntimeError, match="retrieval"):
        retrieval.main(["--data_root", tree])
    F.refuse(_args(None), "anything")                                                             # without the flag nothing is refused
