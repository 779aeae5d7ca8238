"""CPU: the host side of src/models/predict.py — the image-directory loader (src/datasets/image_dir.py), its collate, the command line with its refusals
(all before a model is built or the GPU initialised), the text of predictions.csv, and the new C entries in header and ctypes table."""
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


def gray(path, w, h, seed=0):
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, size=(h, w), dtype=np.uint8)).save(path)


@pytest.fixture
def pictures(tmp_path):
    d = tmp_path / "pics"
    d.mkdir()
    gray(d / "b.PNG", 9, 7, 1)
    gray(d / "a.jpg", 12, 10, 2)
    gray(d / "c.Jpeg", 8, 8, 3)
    gray(d / "d.bmp", 5, 30, 4)
    gray(d / "e.TIF", 16, 3, 5)
    (d / "notes.txt").write_text("not an image")
    (d / "sub").mkdir()
    gray(d / "sub" / "z.png", 4, 4, 6)
    return d


# ------------------------------------------------------------------------------------------------ ImageDir
def test_listing_order_suffixes_and_sizes(pictures):
    from src.datasets.image_dir import ImageDir
    ds = ImageDir(str(pictures), 8)
    assert ds.names == ["a.jpg", "b.PNG", "c.Jpeg", "d.bmp", "e.TIF"] and len(ds) == 5          # sorted by name; the .txt and the sub-directory are ignored
    assert ds.sizes == [(12, 10), (9, 7), (8, 8), (5, 30), (16, 3)]                              # (W, H), from the headers
    px, name = ds[1]
    assert name == "b.PNG" and px.dtype == np.uint8 and px.shape == (7, 9)
    assert np.array_equal(px, np.asarray(Image.open(pictures / "b.PNG").convert("L")))
    assert ds.name_of(4) == "e.TIF"


def test_a_colour_file_is_decoded_to_gray(tmp_path):
    from src.datasets.image_dir import ImageDir
    rgb = np.random.default_rng(0).integers(0, 256, size=(6, 11, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "x.png")
    px, _ = ImageDir(str(tmp_path), 8)[0]
    assert px.shape == (6, 11) and np.array_equal(px, np.asarray(Image.fromarray(rgb).convert("L")))


def test_refusals_by_name(tmp_path):
    from src.datasets.image_dir import ImageDir
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "readme.txt").write_text("x")
    with pytest.raises(RuntimeError, match="holds no image file"):
        ImageDir(str(empty), 8)
    twice = tmp_path / "twice"
    twice.mkdir()
    gray(twice / "scan.png", 8, 8)
    gray(twice / "scan.jpg", 8, 8)
    gray(twice / "other.png", 8, 8)
    with pytest.raises(RuntimeError, match=r"scan\.jpg and scan\.png share the stem 'scan'"):
        ImageDir(str(twice), 8)
    wide = tmp_path / "wide"
    wide.mkdir()
    gray(wide / "fine.png", 8 * 32, 8)                           # a 32x downscale is the limit ...
    assert len(ImageDir(str(wide), 8)) == 1
    gray(wide / "strip.png", 8 * 33, 8)                          # ... 33x is beyond it
    with pytest.raises(RuntimeError, match=r"strip\.png is 264 x 8.*133 taps.*at most 129"):
        ImageDir(str(wide), 8)
    with pytest.raises(RuntimeError, match="--img_size 4 is outside"):
        ImageDir(str(twice), 4)


def test_collate_descriptor_sizes_and_names(pictures):
    from src.datasets.image_dir import ImageDir, ImageDirCollate
    ds = ImageDir(str(pictures), 16)
    buf, desc, labels, (names, hw) = ImageDirCollate(16)([ds[0], ds[3], ds[4]])
    assert labels is None and names == ["a.jpg", "d.bmp", "e.TIF"] and hw == [(10, 12), (30, 5), (3, 16)]
    assert desc.dtype == torch.int32 and desc.tolist() == [[0, 10, 12, -1, 16, 16, 0, 0], [120, 30, 5, -1, 16, 16, 0, 0], [270, 3, 16, -1, 16, 16, 0, 0]]
    assert buf.dtype == torch.uint8 and buf.numel() == 120 + 150 + 48
    assert np.array_equal(buf[120:270].numpy().reshape(30, 5), ds[3][0])


def test_loader_yields_every_image_once_in_name_order(pictures):
    from src.datasets.image_dir import ImageDirModule
    dm = ImageDirModule(str(pictures), 8, batch_size=2, num_workers=0)
    got = [n for _, _, _, (names, _) in dm.loader for n in names]
    assert got == dm.dataset.names and len(dm.loader) == 3
    dm.shutdown()


# ------------------------------------------------------------------------------------------------ command line
def test_split_at_the_double_dash():
    from src.models import predict as P
    own, rest = P.get_args(["--entry", "baselines.segmentation", "--images", "in", "--out", "o", "--no-overlay", "--", "--img_size", "32", "--exp", "e"])
    assert (own.entry, own.images, own.out, own.overlay, own.checkpoint) == ("baselines.segmentation", "in", "o", False, None)
    assert rest == ["--img_size", "32", "--exp", "e"]
    own, rest = P.get_args(["--entry", "dino.classification", "--images", "in", "--out", "o", "--checkpoint", "w.pth"])
    assert own.overlay is True and own.checkpoint == "w.pth" and rest == []
    assert P.split_argv(["a", "--", "b", "--", "c"]) == (["a"], ["b", "--", "c"])


def test_every_supervised_entry_is_known_and_importable_by_name():
    from src.models import predict as P
    models = os.path.join(ROOT, "nextgen-uia_amd", "src", "models")
    on_disk = sorted(f"{d}.{k}" for d in os.listdir(models) for k in ("classification", "segmentation") if os.path.isfile(os.path.join(models, d, k + ".py")))
    assert sorted(f"{f}.{k}" for f, kinds in P.ENTRIES.items() for k in kinds) == on_disk and "clipseg.segmentation" in on_disk
    from src.models.clipseg import segmentation as clipseg
    assert callable(clipseg._batch_prompt)                       # what predict takes from the module for CLIPSeg's per-batch prompt


@pytest.mark.parametrize("entry", ["nope.segmentation", "baselines.fewshot_classification", "biomedclip.fewshot_segmentation", "biomedclip.finetune",
                                   "biomedclip.zero_shot", "biomedclip.retrieval", "clipseg.classification", "baselines", "supervised", ""])
def test_other_entries_are_refused_before_a_model_is_built(entry, monkeypatch, tmp_path):
    from src.models import predict as P
    from src.models.baselines import classification, segmentation
    from src.models.biomedclip import segmentation as bseg

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    for m in (classification, segmentation, bseg):
        monkeypatch.setattr(m, "prepare_model", boom)
    monkeypatch.setattr(P, "load_model", boom)
    before = torch.cuda.is_initialized()                         # (true when GPU tests ran earlier in this process)
    with pytest.raises(ValueError, match=re.escape(f"--entry {entry}:")):
        P.main(["--entry", entry, "--images", str(tmp_path), "--out", str(tmp_path / "o")])
    assert torch.cuda.is_initialized() == before


def _refused(monkeypatch, argv, exc, match):
    from src.models import predict as P
    from src.models.baselines import segmentation

    def boom(*a, **k):
        raise AssertionError("a model was built before the refusal")
    monkeypatch.setattr(segmentation, "prepare_model", boom)
    monkeypatch.setattr(P, "load_model", boom)
    before = torch.cuda.is_initialized()                         # (true when GPU tests ran earlier in this process)
    with pytest.raises(exc, match=match):
        P.main(argv)
    assert torch.cuda.is_initialized() == before


def test_missing_checkpoint_images_and_used_out_are_refused_before_the_gpu(pictures, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    out = tmp_path / "out"
    base = ["--entry", "baselines.segmentation", "--images", str(pictures), "--out", str(out)]
    tail = ["--", "--img_size", "32", "--exp", "e1", "--dataset", "D", "--num_workers", "0"]
    # no runs/e1/D/train/best_model.pth here: the default path is formed from --exp / --dataset and named in the refusal
    _refused(monkeypatch, base + tail, FileNotFoundError, re.escape("runs/e1/D/train/best_model.pth not found"))
    _refused(monkeypatch, base + ["--checkpoint", "w.pth"] + tail, FileNotFoundError, r"checkpoint w\.pth not found")
    assert not out.exists()                                      # nothing was created on the way
    os.makedirs("runs/e1/D/train")
    torch.save({}, "runs/e1/D/train/best_model.pth")
    _refused(monkeypatch, ["--entry", "baselines.segmentation", "--images", str(tmp_path / "absent"), "--out", str(out)] + tail, FileNotFoundError,
             "no such directory")
    out.mkdir()
    (out / "old.png").write_bytes(b"x")
    _refused(monkeypatch, base + tail, FileExistsError, "nothing is overwritten")
    assert os.listdir(out) == ["old.png"]
    # the entry's own refusal (an img_size the UNet cannot take) still comes before a model
    (out / "old.png").unlink()
    _refused(monkeypatch, base + ["--", "--img_size", "40", "--exp", "e1", "--dataset", "D"], ValueError, "multiple of 16")


def test_default_checkpoint_path():
    from src.models import predict as P
    from src.models.baselines import classification
    assert P.default_checkpoint(classification.get_args(["--exp", "x", "--dataset", "BUSI"])) == "runs/x/BUSI/train/best_model.pth"
    a = classification.get_args([])
    assert P.default_checkpoint(a) == f"runs/{a.exp}/{a.dataset}/train/best_model.pth"


# ------------------------------------------------------------------------------------------------ predictions.csv
def test_segmentation_csv_text():
    from src.models import predict as P
    names, sizes = ["a.jpg", "b.png", "c.png"], [(10, 12), (4, 5), (1, 1)]
    stats = np.array([[30, 2, 3, 7, 11, 0, 0, 0], [0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    assert P.seg_csv(names, sizes, stats) == ("name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax\n"
                                              "a.jpg,12,10,30,0.250000,2,3,7,11\n"
                                              "b.png,5,4,0,0.000000,,,,\n"
                                              "c.png,1,1,1,1.000000,0,0,0,0\n")


def test_classification_csv_text():
    from src.models import predict as P
    text = P.cls_csv(["a.jpg", "b.png", "c.png"], [(10, 12), (4, 5), (7, 7)], [[0.25, 0.75], [0.5, 0.5], [1.0, 0.0]])
    assert text == ("name,width,height,p0,p1,predicted\n"
                    "a.jpg,12,10,0.25000000,0.75000000,1\n"
                    "b.png,5,4,0.50000000,0.50000000,0\n"
                    "c.png,7,7,1.00000000,0.00000000,0\n")


# ------------------------------------------------------------------------------------------------ the C entries
def test_new_symbols_are_declared_bound_and_documented():
    from uia_hip import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "uia_hip.h")).read(), flags=re.S)
    for name in ("uia_seg_predict_native", "uia_seg_native_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert len(_lib.PROTOTYPES["uia_seg_predict_native"][1]) == 12
    lib = _lib.lib()
    assert lib.uia_seg_native_workspace_bytes(0) == 0 and lib.uia_seg_native_workspace_bytes(65536) == 0
    assert lib.uia_seg_native_workspace_bytes(1) >= 32 and lib.uia_seg_native_workspace_bytes(65535) >= 65535 * 32


def test_host_checks_run_before_anything_is_enqueued():
    """The launcher's checks need no GPU: every refusal below returns before the first HIP call (the pointers are never followed)."""
    from uia_hip import _lib
    lib = _lib.lib()
    B, S = 2, 8
    desc = np.array([[0, 4, 5, 0, 20, 0, 0, 0], [20, 3, 3, 80, -1, 0, 0, 0]], dtype=np.int32)
    ws_bytes = lib.uia_seg_native_workspace_bytes(B)
    LOG, SRC, OUT, WS, ST = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # addresses that are never dereferenced on a refused call

    def call(d=desc, B=B, S=S, log=LOG, src=SRC, src_bytes=29, out=OUT, out_bytes=89, ws=WS, wsb=ws_bytes, st=ST):
        d = np.ascontiguousarray(d, dtype=np.int32)
        return lib.uia_seg_predict_native(None, B, S, log, src, src_bytes, d.ctypes.data, out, out_bytes, ws, wsb, st), lib.uia_last_error().decode()

    def edit(b, w, v):
        d = desc.copy()
        d[b, w] = v
        return d
    cases = [(dict(B=0), "bad shape"), (dict(B=65536), "bad shape"), (dict(S=7), "bad shape"), (dict(S=1025), "bad shape"), (dict(log=None), "null"),
             (dict(out=None), "null"), (dict(ws=None), "null"), (dict(st=None), "null"), (dict(src=None), "image 0 asks for an overlay but src is null"),
             (dict(wsb=ws_bytes - 1), "workspace"), (dict(d=edit(1, 1, 0)), "image 1 is 0 x 3"), (dict(d=edit(0, 2, 16385)), "image 0 is 4 x 16385"),
             (dict(d=edit(1, 5, 1)), "image 1 has a non-zero reserved"), (dict(d=edit(0, 7, -1)), "image 0 has a non-zero reserved"),
             (dict(d=edit(1, 0, -2)), "image 1 has source offset -2"), (dict(d=edit(0, 0, 10)), "image 0 (offset 10, 4 x 5) leaves the source buffer"),
             (dict(out_bytes=88), "the mask of image 1"), (dict(d=edit(0, 4, 30)), "the overlay of image 0"), (dict(d=edit(0, 3, -1)), "the mask of image 0"),
             (dict(d=edit(1, 3, 79)), "the overlay of image 0 overlaps the mask of image 1"), (dict(d=edit(1, 3, 19)), "the mask of image 0 overlaps the mask of image 1"),
             (dict(out=SRC + 28), "of image 0 overlaps src"), (dict(out=LOG + 1023 - 88), "overlaps logits"), (dict(st=WS), "stats overlaps the workspace"),
             (dict(out=ST + 63), "overlaps stats")]
    for kw, word in cases:
        rc, err = call(**kw)
        assert rc != 0 and word in err and "uia_seg_predict_native" in err, (kw, rc, err)
