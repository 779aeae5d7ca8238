"""CPU: the host side of uia_mask_components (csrc/components.hip) and of the component flags of src/models/predict.py — the yardstick the GPU tests
compare the kernel with (tests/components_reference.py: an explicit-stack flood fill, pinned here against scipy.ndimage.label where scipy imports), every
refusal of the C entry (they come before the first HIP call), the wiring of the symbol, the command line and the text of lesions.csv."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import components_reference as R  # noqa: E402

INT_MAX = 2 ** 31 - 1
SHAPES = [(1, 1), (1, 37), (37, 1), (7, 5), (33, 65), (130, 70)]


# ------------------------------------------------------------------------------------------------ the yardstick
def test_flood_fill_on_a_literal_mask():
    m = np.array([[1, 0, 0, 7, 7],
                  [0, 1, 0, 0, 7],
                  [0, 0, 0, 0, 0],
                  [9, 9, 0, 0, 1]], dtype=np.uint8)
    l4, n4 = R.flood_label(m, 4)
    l8, n8 = R.flood_label(m, 8)
    assert n4 == 5 and n8 == 4
    assert l4.tolist() == [[1, 0, 0, 2, 2], [0, 3, 0, 0, 2], [0, 0, 0, 0, 0], [4, 4, 0, 0, 5]]       # numbered by first pixel
    assert l8.tolist() == [[1, 0, 0, 2, 2], [0, 1, 0, 0, 2], [0, 0, 0, 0, 0], [3, 3, 0, 0, 4]]
    # 8-connected order: areas 3 (first 3), 2 (first 0), 2 (first 15), 1 -> equal areas by the smaller first pixel
    mask, over, stats, rows = R.apply(m, None, min_area=2, keep=2, connectivity=8, max_list=3)
    assert mask.tolist() == [[1, 0, 0, 7, 7], [0, 1, 0, 0, 7], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]] and over is None     # kept pixels keep their bytes
    assert stats.tolist() == [5, 0, 0, 1, 4, 4, 2, 8]
    assert rows.tolist() == [[3, 0, 3, 1, 4, 3, 0, 3], [2, 0, 0, 1, 1, 0, 0, 0], [0] * 8]           # cy = floor(1 / 3), cx = floor(11 / 3); floor(1 / 2) twice
    mask, _, stats, rows = R.apply(m, None, min_area=3, keep=0, connectivity=4, max_list=1)
    assert stats.tolist() == [3, 0, 3, 1, 4, 5, 1, 8] and rows.tolist() == [[3, 0, 3, 1, 4, 3, 0, 3]]
    _, _, stats, rows = R.apply(np.zeros((3, 4), np.uint8), None, keep=1, max_list=2)
    assert stats.tolist() == [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0] and not rows.any()
    g = np.arange(20, dtype=np.uint8).reshape(4, 5)
    over = np.stack([g, np.maximum(g, (m != 0) * np.uint8(255)), g], axis=-1)
    _, after, _, _ = R.apply(m, over, keep=1, connectivity=8)
    gone = (m != 0) & ~np.isin(np.arange(20).reshape(4, 5), [3, 4, 9])
    assert np.array_equal(after[gone], np.stack([g[gone]] * 3, axis=-1)) and np.array_equal(after[~gone], over[~gone])


def test_checkerboard_ties_go_to_the_first_pixels():
    m = R.patterns(7, 5)["checkerboard"]
    _, _, stats, rows = R.apply(m, None, keep=3, connectivity=4, max_list=5)
    assert stats[5] == 18 and stats[6] == 3 and stats[0] == 3 and stats[7] == 18
    assert rows[:, 5].tolist() == [0, 2, 4, 0, 0] and rows[:3, 0].tolist() == [1, 1, 1]
    _, _, stats, _ = R.apply(m, None, keep=3, connectivity=8)
    assert stats[5] == 1 and stats[6] == 1 and stats[0] == 18


@pytest.mark.parametrize("shape", SHAPES + [(300, 517)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_flood_fill_agrees_with_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    pats = R.patterns(*shape)
    if shape == (300, 517):
        pats = {k: pats[k] for k in ("spiral", "checkerboard", "random0.5", "corner")}
    for name, m in pats.items():
        for conn in (4, 8):
            labels, n = R.flood_label(m, conn)
            theirs, count = ndimage.label(m != 0, structure=np.ones((3, 3), int) if conn == 8 else None)
            assert n == count, (name, conn)
            assert np.array_equal(labels > 0, m != 0)
            assert sorted(np.bincount(labels.ravel())[1:].tolist()) == sorted(np.bincount(theirs.ravel())[1:].tolist()), (name, conn)


def test_patterns_are_what_their_names_say():
    for H, W in ((33, 65), (130, 70)):
        p = R.patterns(H, W)
        assert R.flood_label(p["spiral"], 4)[1] == 1 and R.flood_label(p["spiral"], 8)[1] == 1 and int(p["spiral"].astype(bool).sum()) > H * W // 3
        assert R.flood_label(p["corner"], 4)[1] == 2 and R.flood_label(p["corner"], 8)[1] == 1
        assert R.flood_label(p["checkerboard"], 8)[1] == 1 and R.flood_label(p["checkerboard"], 4)[1] == (H * W + 1) // 2
        assert R.flood_label(p["comb"], 4)[1] == 1 and R.flood_label(p["rings"], 8)[1] > 5
        assert set(np.unique(p["values"])) - {0, 255}


# ------------------------------------------------------------------------------------------------ the C entry
NAMES = ("uia_mask_components", "uia_mask_components_workspace_bytes")


def test_symbol_is_declared_exported_typed_wrapped_and_documented():
    from uia_hip import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uia_hip.h")).read(), flags=re.S)
    kernels = open(os.path.join(ROOT, "nextgen-uia_amd", "csrc", "uia_kernels.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.PROTOTYPES and name in doc, name
        getattr(lib, name)
    assert "uia_mask_components_launch" in kernels and "uia_mask_components_ws_bytes" in kernels
    assert len(_lib.PROTOTYPES["uia_mask_components"][1]) == 10
    assert callable(ops.mask_components) and ops.MASK_COMPONENTS_DESC == 8 and "mask_components" in doc
    for B, px in ((0, 10), (65536, 10), (1, 0), (1, 2 ** 31), (1, -5)):
        assert lib.uia_mask_components_workspace_bytes(B, px) == 0, (B, px)
    one, two = lib.uia_mask_components_workspace_bytes(1, 1000), lib.uia_mask_components_workspace_bytes(1, 2000)
    assert one >= 8 * 1000 and 8000 <= two - one <= 8000 + 512                       # 8 bytes per pixel
    assert lib.uia_mask_components_workspace_bytes(65535, 2 ** 31 - 1) > 8 * (2 ** 31 - 1)


def test_every_refusal_comes_before_anything_is_enqueued():
    """The launcher's checks need no GPU: every refusal below returns before the first HIP call (the pointers are never followed)."""
    from uia_hip import _lib
    lib = _lib.lib()
    B = 2
    # image 0: 4 x 5 mask at 1, overlay at 21 .. 81; image 1: 3 x 3 mask at 81 .. 90, no overlay
    desc = np.array([[1, 4, 5, 21, 0, 0, 8, 0], [81, 3, 3, -1, 2, 1, 4, 0]], dtype=np.int32)
    need = lib.uia_mask_components_workspace_bytes(B, 29)
    BUF, WS, ST, LI = 0x100000, 0x200000, 0x300000, 0x400000                 # addresses that are never dereferenced on a refused call
    assert 0 < need < 0x100000

    def call(d=desc, B=B, buf=BUF, buf_bytes=90, ws=WS, wsb=need, st=ST, li=LI, max_list=4):
        d = np.ascontiguousarray(d, dtype=np.int32)
        return lib.uia_mask_components(None, B, buf, buf_bytes, d.ctypes.data, ws, wsb, st, li, max_list), lib.uia_last_error().decode()

    def edit(b, w, v):
        d = desc.copy()
        d[b, w] = v
        return d
    cases = [(dict(B=0), "bad shape"), (dict(B=65536), "bad shape"), (dict(d=edit(1, 1, 0)), "image 1 is 0 x 3"), (dict(d=edit(0, 2, 16385)), "image 0 is 4 x 16385"),
             (dict(buf=None), "null"), (dict(d=None), "null"), (dict(ws=None), "null"), (dict(st=None), "null"), (dict(li=None), "null list with max_list=4"),
             (dict(max_list=-1), "max_list=-1"), (dict(max_list=33), "max_list=33"), (dict(d=edit(1, 6, 6)), "image 1 has connectivity 6"),
             (dict(d=edit(0, 6, 0)), "image 0 has connectivity 0"), (dict(d=edit(0, 4, -1)), "image 0 has min_area -1"), (dict(d=edit(1, 5, -3)), "keep -3"),
             (dict(d=edit(1, 7, 1)), "image 1 has a non-zero reserved"), (dict(buf_bytes=89), "the mask of image 1"), (dict(d=edit(0, 0, -1)), "the mask of image 0"),
             (dict(d=edit(0, 3, 31)), "the overlay of image 0"), (dict(d=edit(0, 3, -2)), "image 0 has overlay offset -2"),
             (dict(d=edit(1, 0, 80)), "the overlay of image 0 overlaps the mask of image 1"), (dict(d=edit(0, 0, 2)), "the mask of image 0 overlaps the overlay of image 0"),
             (dict(d=edit(1, 3, 0), buf_bytes=200), "overlaps"), (dict(st=BUF + 88), "of image 1 overlaps stats"), (dict(li=BUF - 4), "overlaps list"),
             (dict(ws=BUF + 88), "overlaps the workspace"), (dict(st=WS + need - 4), "stats overlaps the workspace"), (dict(li=ST + 60), "stats overlaps list"),
             (dict(li=WS - 4), "list overlaps the workspace"), (dict(wsb=need - 1), "workspace of"), (dict(buf_bytes=2 ** 31), "a buffer of")]
    for kw, word in cases:
        if kw.get("d", 0) is None:
            rc, err = lib.uia_mask_components(None, B, BUF, 90, None, WS, need, ST, LI, 4), lib.uia_last_error().decode()
        else:
            rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_mask_components" in err, (kw, rc, err)
    # a list pointer is not looked at when max_list is 0 ... but everything else still is
    rc, err = call(li=None, max_list=0, d=edit(0, 6, 5))
    assert rc != 0 and "image 0 has connectivity 5" in err


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["--entry", "baselines.segmentation", "--images", "in", "--out", "o"]


def test_component_flags_and_their_defaults():
    from src.models import predict as P
    own, rest = P.get_args(BASE)
    assert (own.min_area, own.keep_largest, own.connectivity, own.lesions) == (0, 0, 8, 0) and rest == []
    own, rest = P.get_args(BASE + ["--min_area", "50", "--keep_largest", "1", "--connectivity", "4", "--lesions", "4", "--", "--img_size", "32"])
    assert (own.min_area, own.keep_largest, own.connectivity, own.lesions) == (50, 1, 4, 4) and rest == ["--img_size", "32"]
    P.check_components(own, "segmentation")
    with pytest.raises(SystemExit):
        P.get_args(BASE + ["--connectivity", "6"])
    for bad, word in ((["--lesions", "33"], "--lesions 33"), (["--lesions", "-1"], "--lesions -1"), (["--min_area", "-2"], "--min_area -2"),
                      (["--keep_largest", "-1"], "--keep_largest -1")):
        with pytest.raises(ValueError, match=re.escape(word)):
            P.check_components(P.get_args(BASE + bad)[0], "segmentation")


@pytest.mark.parametrize("flags", [["--min_area", "5"], ["--keep_largest", "1"], ["--connectivity", "4"], ["--lesions", "3"], ["--keep_largest", "2", "--lesions", "2"]],
                         ids=lambda f: f[0])
def test_component_flags_are_refused_for_classification_before_the_gpu(flags, monkeypatch, tmp_path):
    from src.models import predict as P
    from src.models.baselines import classification

    def boom(*a, **k):
        raise AssertionError("the entry was used before the refusal")
    monkeypatch.setattr(classification, "prepare_model", boom)
    monkeypatch.setattr(classification, "get_args", boom)
    monkeypatch.setattr(P, "load_model", boom)
    monkeypatch.setattr(P, "run", boom)
    before = torch.cuda.is_initialized()                         # (true when GPU tests ran earlier in this process)
    with pytest.raises(ValueError, match=re.escape(f"--entry baselines.classification: {', '.join(flags[::2])} filter segmentation masks")):
        P.main(["--entry", "baselines.classification", "--images", str(tmp_path), "--out", str(tmp_path / "o")] + flags)
    assert torch.cuda.is_initialized() == before and not (tmp_path / "o").exists()


def test_lesions_csv_text():
    from src.models import predict as P
    lists = [np.array([[120, 3, 4, 20, 30, 3 * 64 + 9, 11, 17], [7, 0, 0, 1, 5, 0, 0, 2], [0] * 8], dtype=np.int32),
             np.zeros((3, 8), dtype=np.int32),
             np.array([[1, 5, 6, 5, 6, 46, 5, 6], [1, 7, 0, 7, 0, 56, 7, 0], [1, 7, 7, 7, 7, 63, 7, 7]], dtype=np.int32)]
    assert P.lesions_csv(["a.jpg", "b.png", "c.png"], lists) == ("name,lesion,area,ymin,xmin,ymax,xmax,cy,cx\n"
                                                                 "a.jpg,1,120,3,4,20,30,11,17\n"
                                                                 "a.jpg,2,7,0,0,1,5,0,2\n"
                                                                 "c.png,1,1,5,6,5,6,5,6\n"
                                                                 "c.png,2,1,7,0,7,0,7,0\n"
                                                                 "c.png,3,1,7,7,7,7,7,7\n")
    assert P.lesions_csv([], []) == "name,lesion,area,ymin,xmin,ymax,xmax,cy,cx\n"


def test_predictions_csv_is_unchanged_for_the_old_statistics_rows():
    from src.models import predict as P
    names, sizes = ["a.jpg", "b.png", "c.png"], [(10, 12), (4, 5), (1, 1)]
    old = np.array([[30, 2, 3, 7, 11, 0, 0, 0], [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    text = ("name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax\n"
            "a.jpg,12,10,30,0.250000,2,3,7,11\n"
            "b.png,5,4,0,0.000000,,,,\n"
            "c.png,1,1,1,1.000000,0,0,0,0\n")
    assert P.seg_csv(names, sizes, old) == text
    new = old.copy()
    new[:, 5:] = [[4, 1, 55], [2, 0, 9], [1, 1, 1]]                 # components found, kept, foreground before: not columns of predictions.csv
    assert P.seg_csv(names, sizes, new) == text
