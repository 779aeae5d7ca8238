"""CPU: the host side of prediction ensembles — the flags of src/models/predict.py with their refusals (all before a model is built or the GPU initialised),
the member order, the extended predictions.csv, NativeMaskWriter.layout with the two maps, and the two new C entries in header, library, ctypes table and
INTEGRATION.md's stub, with the launcher's own refusals (they return before the first HIP call)."""
import ctypes as C
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

Image = pytest.importorskip("PIL.Image")

INT_MAX = 2 ** 31 - 1
BASE = ["--entry", "baselines.segmentation", "--images", "in", "--out", "o"]
OLD_SEG_HEADER = "name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax"


# ------------------------------------------------------------------------------------------------ the flags
def test_flag_table_and_defaults():
    from src.models import predict as P
    own, rest = P.get_args(BASE + ["--", "--exp", "e"])
    assert (own.ensemble, own.tta, own.threshold, own.prob, own.spread) == (None, "none", 0.5, False, False) and rest == ["--exp", "e"]
    assert P.ensemble_given(own) == [] and P.members_of(own) == [(0, 0)]
    # ... and the old arguments are what they were
    assert (own.entry, own.images, own.out, own.checkpoint, own.overlay, own.min_area, own.keep_largest, own.connectivity, own.lesions) == \
        ("baselines.segmentation", "in", "o", None, True, 0, 0, 8, 0)
    assert P.SEG_HEADER == OLD_SEG_HEADER and P.CLS_HEADER == "name,width,height,p0,p1,predicted"
    assert P.TTA_FLIPS == {"none": (0,), "hflip": (0, 1), "vflip": (0, 2), "flips": (0, 1, 2, 3)} and P.MAX_MEMBERS == 16
    own, _ = P.get_args(BASE + ["--ensemble", "b.pth", "c.pth", "--tta", "hflip", "--threshold", "0.35", "--prob", "--spread", "--no-overlay"])
    assert (own.ensemble, own.tta, own.threshold, own.prob, own.spread, own.overlay) == (["b.pth", "c.pth"], "hflip", 0.35, True, True, False)
    assert P.ensemble_given(own) == ["--ensemble", "--tta", "--threshold", "--prob", "--spread"]
    for flag, argv in (("--ensemble", ["--ensemble", "x"]), ("--tta", ["--tta", "vflip"]), ("--threshold", ["--threshold", "0.4"]), ("--prob", ["--prob"]),
                       ("--spread", ["--spread"])):
        assert P.ensemble_given(P.get_args(BASE + argv)[0]) == [flag]
    with pytest.raises(SystemExit):
        P.get_args(BASE + ["--tta", "rot90"])
    with pytest.raises(SystemExit):
        P.get_args(BASE + ["--ensemble"])
    doc = P.__doc__
    for word in ("--ensemble", "--tta", "--threshold", "--prob", "--spread", "probs/<stem>.png", "spread/<stem>.png", "mean_foreground_probability", "mean_spread"):
        assert word in doc, word


def test_member_order_is_checkpoints_by_flips():
    from src.models import predict as P
    own, _ = P.get_args(BASE + ["--ensemble", "b", "c", "--tta", "flips"])
    assert P.members_of(own) == [(c, f) for c in (0, 1, 2) for f in (0, 1, 2, 3)]
    own, _ = P.get_args(BASE + ["--tta", "vflip"])
    assert P.members_of(own) == [(0, 0), (0, 2)]
    own, _ = P.get_args(BASE + ["--ensemble", "b", "--tta", "hflip"])
    assert P.members_of(own) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    from uia_hip import ops
    assert ops.seg_flip_bits([f for _, f in P.members_of(own)]) == 0b01000100 and ops.seg_flip_bits([0, 1, 2, 3]) == 0b11100100 and ops.SEG_NATIVE_ENS_MAX_K == 16
    for bad in ([], [0] * 17, [4], [-1]):
        with pytest.raises(ops.UiaError, match="flips"):
            ops.seg_flip_bits(bad)


def _refused(monkeypatch, argv, exc, match):
    from src.models import predict as P
    from src.models.baselines import classification, segmentation

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    for m in (classification, segmentation):
        monkeypatch.setattr(m, "prepare_model", boom)
    monkeypatch.setattr(P, "load_model", boom)
    before = torch.cuda.is_initialized()                         # (true when GPU tests ran earlier in this process)
    with pytest.raises(exc, match=match):
        P.main(argv)
    assert torch.cuda.is_initialized() == before


def test_more_than_sixteen_members_are_refused_before_the_entry_is_imported(monkeypatch):
    import importlib
    from src.models import predict as P

    def no_import(name, *a, **k):
        raise AssertionError(f"{name} was imported before the refusal")
    monkeypatch.setattr(importlib, "import_module", no_import)
    many = ["--ensemble"] + [f"s{i}.pth" for i in range(4)]
    with pytest.raises(ValueError, match=r"5 checkpoints x 4 flips = 20 members, at most 16"):
        P.main(BASE + many + ["--tta", "flips"])
    with pytest.raises(ValueError, match=r"17 checkpoints x 1 flips = 17 members"):
        P.main(BASE + ["--ensemble"] + [f"s{i}.pth" for i in range(16)])
    with pytest.raises(ValueError, match=r"--threshold 1\.0"):
        P.main(BASE + ["--threshold", "1.0"])
    with pytest.raises(ValueError, match=r"--threshold 0\.0"):
        P.main(BASE + ["--threshold", "0"])
    own, _ = P.get_args(BASE + ["--ensemble", "a", "b", "c", "--tta", "flips"])      # 16 members pass
    P.check_ensemble(own, "segmentation")
    assert len(P.members_of(own)) == 16


@pytest.mark.parametrize("argv,flags", [(["--threshold", "0.4"], "--threshold"), (["--prob"], "--prob"), (["--spread"], "--spread"),
                                        (["--prob", "--spread", "--threshold", "0.3"], "--threshold, --prob, --spread")])
def test_segmentation_only_flags_are_refused_for_classification_by_name(argv, flags, monkeypatch, tmp_path):
    _refused(monkeypatch, ["--entry", "baselines.classification", "--images", str(tmp_path), "--out", str(tmp_path / "o")] + argv, ValueError,
             re.escape(f"--entry baselines.classification: {flags} shape segmentation masks"))
    from src.models import predict as P
    own, _ = P.get_args(["--entry", "baselines.classification", "--images", "i", "--out", "o", "--ensemble", "b.pth", "--tta", "flips"])
    P.check_ensemble(own, "classification")                      # --ensemble and --tta are for both kinds


def test_a_missing_ensemble_file_is_refused_before_the_gpu(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pics = tmp_path / "pics"
    pics.mkdir()
    Image.fromarray(np.zeros((8, 8), dtype=np.uint8)).save(pics / "a.png")
    torch.save({}, "first.pth")
    torch.save({}, "second.pth")
    out = tmp_path / "out"
    tail = ["--", "--img_size", "32", "--exp", "e1", "--dataset", "D", "--num_workers", "0"]
    _refused(monkeypatch, ["--entry", "baselines.segmentation", "--images", str(pics), "--out", str(out), "--checkpoint", "first.pth", "--ensemble", "second.pth",
                           "third.pth"] + tail, FileNotFoundError, r"--ensemble third\.pth not found")
    _refused(monkeypatch, ["--entry", "baselines.classification", "--images", str(pics), "--out", str(out), "--checkpoint", "first.pth", "--ensemble", "nope.pth"] + tail,
             FileNotFoundError, r"--ensemble nope\.pth not found")
    assert not out.exists()                                      # nothing was created on the way


# ------------------------------------------------------------------------------------------------ predictions.csv
def test_extended_segmentation_csv_text():
    from src.models import predict as P
    names, sizes = ["a.jpg", "b.png", "c.png"], [(10, 12), (4, 5), (1, 1)]
    stats = np.array([[30, 2, 3, 7, 11, 0, 0, 0], [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    sums = np.array([[30 * 204, 120 * 51], [0, 255 * 20], [255, 0]], dtype=np.int64)
    assert P.seg_csv(names, sizes, stats, sums) == (OLD_SEG_HEADER + ",mean_foreground_probability,mean_spread\n"
                                                    "a.jpg,12,10,30,0.250000,2,3,7,11,0.800000,0.200000\n"
                                                    "b.png,5,4,0,0.000000,,,,,,1.000000\n"
                                                    "c.png,1,1,1,1.000000,0,0,0,0,1.000000,0.000000\n")
    # behind the component filter word 7 is the foreground before it: the mean is over the unfiltered mask, also when the filter emptied the mask
    filtered = np.array([[20, 2, 3, 7, 11, 2, 1, 30], [0, INT_MAX, INT_MAX, -1, -1, 1, 0, 4], [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0]], dtype=np.int32)
    sums = np.array([[30 * 204, 0], [4 * 153, 0], [0, 0]], dtype=np.int64)
    assert P.seg_csv(names, sizes, filtered, sums, filtered=True) == (OLD_SEG_HEADER + ",mean_foreground_probability,mean_spread\n"
                                                                      "a.jpg,12,10,20,0.166667,2,3,7,11,0.800000,0.000000\n"
                                                                      "b.png,5,4,0,0.000000,,,,,0.600000,0.000000\n"
                                                                      "c.png,1,1,0,0.000000,,,,,,0.000000\n")
    # a sum beyond 32 bits
    big = np.array([[2 ** 24, 0, 0, 4095, 4095, 0, 0, 0]], dtype=np.int32)
    assert P.seg_csv(["x.png"], [(4096, 4096)], big, np.array([[255 * 2 ** 24, 255 * 2 ** 23]], dtype=np.int64)).endswith(",1.000000,0.500000\n")


def test_without_sums_the_csv_is_the_old_one():
    from src.models import predict as P
    names, sizes = ["a.jpg", "b.png"], [(10, 12), (4, 5)]
    stats = np.array([[30, 2, 3, 7, 11, 0, 0, 0], [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0]], dtype=np.int32)
    assert P.seg_csv(names, sizes, stats) == OLD_SEG_HEADER + "\na.jpg,12,10,30,0.250000,2,3,7,11\nb.png,5,4,0,0.000000,,,,\n"


# ------------------------------------------------------------------------------------------------ NativeMaskWriter.layout
def test_layout_places_the_maps_behind_the_overlay():
    from src.utils.viz import NativeMaskWriter
    sizes = [(3, 5), (2, 2)]
    assert NativeMaskWriter.layout(sizes, True) == ([(0, 15), (60, 64)], 76)                   # as before
    assert NativeMaskWriter.layout(sizes, False) == ([(0, -1), (15, -1)], 19)
    assert NativeMaskWriter.layout(sizes, True, prob=True, spread=True) == ([(0, 15, 60, 75), (90, 94, 106, 110)], 114)
    assert NativeMaskWriter.layout(sizes, True, prob=True) == ([(0, 15, 60, -1), (75, 79, 91, -1)], 95)
    assert NativeMaskWriter.layout(sizes, False, spread=True) == ([(0, -1, -1, 15), (30, -1, -1, 34)], 38)
    assert NativeMaskWriter.layout(sizes, False, True, False) == ([(0, -1, 15, -1), (30, -1, 34, -1)], 38)


def test_writer_refuses_a_threshold_outside_the_open_interval(tmp_path):
    from src.utils.viz import NativeMaskWriter
    for t in (0.0, 1.0, -1, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            NativeMaskWriter(tmp_path / "o", threshold=t, device="cpu")
    assert not (tmp_path / "o").exists()


# ------------------------------------------------------------------------------------------------ the C entries
NAMES = ("uia_seg_predict_native_ens", "uia_seg_native_ens_workspace_bytes")


def test_new_symbols_are_declared_exported_bound_and_documented():
    from uia_hip import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uia_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.PROTOTYPES and name in doc and hasattr(handle, name), name
    assert len(_lib.PROTOTYPES["uia_seg_predict_native_ens"][1]) == 16
    # INTEGRATION.md's ctypes stub is the table's row, type for type
    for name in NAMES:
        m = re.search(rf"lib\.{name}\.argtypes = (.*?)`", doc, flags=re.S)
        assert m, name
        assert eval(m.group(1).replace("\n", " "), {"C": C}) == list(_lib.PROTOTYPES[name][1]), name
    assert _lib.PROTOTYPES["uia_seg_native_ens_workspace_bytes"][0] is C.c_size_t and _lib.PROTOTYPES["uia_seg_predict_native_ens"][0] is C.c_int
    kernels = open(os.path.join(ROOT, "nextgen-uia_amd", "csrc", "uia_kernels.h")).read()
    assert "uia_seg_predict_native_ens_launch" in kernels and os.path.isfile(os.path.join(ROOT, "nextgen-uia_amd", "csrc", "seg_native_ens.hip"))
    assert callable(ops.seg_predict_native_ens) and callable(ops.seg_native_ens_workspace)
    lib = _lib.lib()
    assert lib.uia_seg_native_ens_workspace_bytes(0) == 0 and lib.uia_seg_native_ens_workspace_bytes(65536) == 0
    assert lib.uia_seg_native_ens_workspace_bytes(1) >= 32 and lib.uia_seg_native_ens_workspace_bytes(65535) >= 65535 * 32


def test_host_checks_run_before_anything_is_enqueued():
    """The launcher's checks need no GPU: every refusal below returns before the first HIP call (the pointers are never followed)."""
    from uia_hip import _lib
    lib = _lib.lib()
    K, B, S = 2, 2, 8
    # image 0: 4 x 5, mask 0..20, overlay 20..80, probability 80..100, spread 104..124; image 1: 3 x 3, mask 124..133, no overlay, probability 136..145
    desc = np.array([[0, 4, 5, 0, 20, 80, 104, 0], [20, 3, 3, 124, -1, 136, -1, 0]], dtype=np.int32)
    ws_bytes = lib.uia_seg_native_ens_workspace_bytes(B)
    LOG, SRC, OUT, WS, ST, SM = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # addresses that are never dereferenced on a refused call

    def call(d=desc, K=K, B=B, S=S, log=LOG, flips=0b0100, t=0.5, src=SRC, src_bytes=29, out=OUT, out_bytes=145, ws=WS, wsb=ws_bytes, st=ST, sm=SM):
        d = np.ascontiguousarray(d, dtype=np.int32)
        rc = lib.uia_seg_predict_native_ens(None, K, B, S, log, flips, t, src, src_bytes, d.ctypes.data, out, out_bytes, ws, wsb, st, sm)
        return rc, lib.uia_last_error().decode()

    def edit(b, w, v):
        d = desc.copy()
        d[b, w] = v
        return d
    cases = [(dict(B=0), "bad shape"), (dict(B=65536), "bad shape"), (dict(S=7), "bad shape"), (dict(S=1025), "bad shape"), (dict(log=None), "null"),
             (dict(out=None), "null"), (dict(ws=None), "null"), (dict(st=None), "null"), (dict(src=None), "image 0 asks for an overlay but src is null"),
             (dict(wsb=ws_bytes - 1), "workspace"), (dict(d=edit(1, 1, 0)), "image 1 is 0 x 3"), (dict(d=edit(0, 2, 16385)), "image 0 is 4 x 16385"),
             (dict(d=edit(1, 7, 1)), "image 1 has a non-zero reserved"), (dict(d=edit(0, 7, -1)), "image 0 has a non-zero reserved"),
             (dict(d=edit(1, 0, -2)), "image 1 has source offset -2"), (dict(d=edit(0, 0, 10)), "image 0 (offset 10, 4 x 5) leaves the source buffer"),
             (dict(d=edit(0, 5, -2)), "image 0 has source offset 0, overlay offset 20, probability offset -2"), (dict(d=edit(1, 6, -7)), "spread offset -7"),
             (dict(d=edit(1, 3, 137)), "the mask of image 1"), (dict(d=edit(0, 4, 100)), "the overlay of image 0"), (dict(d=edit(0, 3, -1)), "the mask of image 0"),
             (dict(d=edit(1, 3, 79)), "the overlay of image 0 overlaps the mask of image 1"), (dict(d=edit(1, 3, 19)), "the mask of image 0 overlaps the mask of image 1"),
             (dict(out=SRC + 28), "of image 0 overlaps src"), (dict(out=LOG + 2047 - 144), "overlaps logits"), (dict(st=WS), "stats overlaps the workspace"),
             (dict(sm=WS + 8), "sums overlaps the workspace"), (dict(sm=ST + 56), "stats overlaps sums"), (dict(sm=LOG + 8), "logits overlaps sums"),
             (dict(sm=SM + 4), "8-byte aligned"), (dict(log=LOG + 2), "4-byte aligned"),
             (dict(K=0), "K=0 members"), (dict(K=17), "K=17 members"), (dict(K=1), "flips=0x4 has bits at or above 2 K = 2"), (dict(flips=0x10), "flips=0x10"),
             (dict(t=0.0), "threshold 0"), (dict(t=1.0), "threshold 1"), (dict(t=1.5), "threshold 1.5"), (dict(t=float("nan")), "threshold"),
             (dict(out_bytes=144), "the probability map of image 1 (offset 136, 3 x 3) leaves the output buffer of 144 bytes"),
             (dict(d=edit(0, 6, 126)), "the spread map of image 0 (offset 126, 4 x 5) leaves"),
             (dict(d=edit(0, 5, 10)), "the mask of image 0 overlaps the probability map of image 0"),
             (dict(d=edit(0, 5, 61)), "the overlay of image 0 overlaps the probability map of image 0"),
             (dict(d=edit(0, 5, 90)), "the probability map of image 0 overlaps the spread map of image 0"),
             (dict(d=edit(1, 6, 128)), "the mask of image 1 overlaps the spread map of image 1"),
             (dict(d=edit(1, 5, 99)), "the probability map of image 0 overlaps the probability map of image 1"),
             (dict(src=OUT + 80), "the probability map of image 0 overlaps src"), (dict(log=OUT + 136), "the probability map of image 1 overlaps logits"),
             (dict(st=OUT + 104), "the spread map of image 0 overlaps stats"), (dict(sm=OUT + 80), "the probability map of image 0 overlaps sums"),
             (dict(ws=OUT + 136), "the probability map of image 1 overlaps the workspace")]
    for kw, word in cases:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_seg_predict_native_ens" in err, (kw, rc, err)
    rc, err = call(K=16, flips=0xFFFFFFFF, log=None)             # sixteen members use every flip bit: the refusal is the null pointer's, not the flips'
    assert rc != 0 and "null" in err
