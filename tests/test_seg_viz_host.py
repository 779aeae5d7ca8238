"""Host side (no GPU) of the segmentation pictures and of the three CLIP-family segmentation entries: the numpy restatement against what the reference's own
visualize_seg wrote (tests/golden/seg_viz_cases.npz, tools/gen_seg_viz_golden.py), the PNG writer, the command lines against the reference's tables
(tests/golden/reference_seg_cli_tables.json, tools/gen_seg_cli_tables.py), the datasets' name_of and the --viz flag."""
import ast
import importlib
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seg_viz_reference as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEG_ENTRIES = ["baselines", "biomedclip", "clip", "clipseg", "dino", "metaclip", "unimedclip"]


# ------------------------------------------------------------------------------------------------ restatement against the reference's files
def fixture_cases():
    z = np.load(os.path.join(GOLDEN, "seg_viz_cases.npz"))
    n = len({k.split("_")[0] for k in z.files})
    return [{f: z[f"c{c}_{f}"] for f in ("logits", "images", "labels", "mask", "overlay", "pred")} for c in range(n)]


def test_restatement_equals_what_the_reference_wrote():
    cases = fixture_cases()
    assert len(cases) == 4
    seen = set()
    for c in cases:
        mask, overlay, pred = R.seg_viz(c["logits"], c["images"], c["labels"])
        assert np.array_equal(mask, c["mask"]) and np.array_equal(overlay, c["overlay"]) and np.array_equal(pred, c["pred"])
        seen.add((c["logits"].shape[-1], c["images"].shape[1], str(c["labels"].dtype)))
        # what the fixture claims to hold: no NaN, no pixel outside [0, 1], an empty and a full label, a tie and an infinity in the logits
        assert not np.isnan(c["logits"]).any() and c["images"].min() >= 0.0 and c["images"].max() == 1.0
        assert not c["labels"][1].any() and c["labels"][2].all()
        assert (c["logits"][:, 0] == c["logits"][:, 1]).any() and np.isinf(c["logits"]).any()
    assert seen == {(37, 3, "float32"), (37, 1, "uint8"), (5, 3, "uint8"), (5, 1, "float32")}
    big = cases[0]["overlay"][..., 2]
    assert set(np.unique(big)) == set(range(256))                # every grey level is in the picture


def test_every_level_truncates_to_itself_and_the_clamp_holds():
    a = np.arange(256, dtype=np.float32) / np.float32(255)
    b = (torch.arange(256, dtype=torch.uint8).float() / 255.0).numpy()
    assert np.array_equal(R.grey(a), np.arange(256)) and np.array_equal(R.grey(b), np.arange(256))
    x = np.float32([-1.0, -0.0, 0.999999, 1.0, 1.0000001, 7.0, np.inf, -np.inf, np.nan, 0.5])
    assert R.grey(x).tolist() == [0, 0, 254, 255, 255, 255, 255, 0, 0, 127]


def test_class1_is_torch_argmax():
    inf, nan = float("inf"), float("nan")
    pairs = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (inf, inf), (-inf, -inf), (1.0, 2.0), (2.0, 1.0), (nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (inf, nan),
             (-inf, inf), (inf, -inf)]
    lg = torch.tensor(pairs, dtype=torch.float32).T.reshape(1, 2, 1, len(pairs))
    assert np.array_equal(R.class1(lg.numpy()), (lg.argmax(dim=1) == 1).numpy())


# ------------------------------------------------------------------------------------------------ the PNG writer
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 37), (1, 1, 3), (5, 7, 3), (37, 37, 3)])
def test_write_png_round_trip(tmp_path, shape):
    from src.utils.viz import write_png
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    path = tmp_path / "a.png"
    n = write_png(str(path), a)
    data = path.read_bytes()
    assert n == len(data) and data[:8] == b"\x89PNG\r\n\x1a\n"
    # IHDR: 13 bytes, width, height, depth 8, colour type 0 / 2, no interlace; its CRC; one IDAT; IEND closes the file
    assert struct.unpack(">I", data[8:12])[0] == 13 and data[12:16] == b"IHDR"
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", data[16:29])
    assert (w, h, depth, colour, comp, filt, lace) == (shape[1], shape[0], 8, 2 if len(shape) == 3 else 0, 0, 0, 0)
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29]) & 0xFFFFFFFF
    assert data.count(b"IDAT") >= 1 and data[33 + 4:33 + 8] == b"IDAT"
    assert data[-12:] == struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND") & 0xFFFFFFFF)
    assert np.array_equal(R.decode_png(data), a)                 # every chunk's CRC is checked in there
    n_idat = struct.unpack(">I", data[33:37])[0]
    assert 33 + 12 + n_idat + 12 == len(data)                    # exactly one IDAT between IHDR and IEND
    write_png(str(path), torch.from_numpy(a))                    # tensors are taken too
    assert np.array_equal(R.decode_png(path.read_bytes()), a)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 37), (1, 1, 3), (5, 7, 3), (37, 37, 3)])
def test_write_png_is_read_by_pil_pixel_for_pixel(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    from src.utils.viz import write_png
    a = np.random.default_rng(1 + sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    write_png(str(tmp_path / "a.png"), a)
    with Image.open(tmp_path / "a.png") as im:
        assert im.mode == ("RGB" if len(shape) == 3 else "L")
        assert np.array_equal(np.asarray(im), a)


def test_write_png_refuses_what_it_cannot_write(tmp_path):
    from src.utils.viz import write_png
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((4,), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "bad.png"), bad)


def test_file_names_follow_the_reference():
    from src.utils.viz import png_names
    assert png_names("a/b/case_007.png") == ("case_007.png", "case_007_overlay.png", "case_007_pred.png")
    assert png_names("scan.v2.jpg") == ("scan.v2.png", "scan.v2_overlay.png", "scan.v2_pred.png")


# ------------------------------------------------------------------------------------------------ command lines
def _argparse_table(path):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument" and node.args and isinstance(node.args[0], ast.Constant):
            out[node.args[0].value] = {k.arg: ast.unparse(k.value) for k in node.keywords if k.arg in ("default", "action", "choices")}
    return out


@pytest.mark.parametrize("entry", ["clip/segmentation.py", "metaclip/segmentation.py", "unimedclip/segmentation.py"])
def test_every_reference_flag_is_there_with_its_default(entry):
    """The argparse tables of reference and build compared syntactically (flag set, default / action / choices expressions); `--device` is the one deliberate
    difference (decided without a HIP call, src/utils/tools.default_device)."""
    ref = json.load(open(os.path.join(GOLDEN, "reference_seg_cli_tables.json")))[entry]
    got = _argparse_table(os.path.join(ROOT, "nextgen-uia_amd/src/models", entry))
    assert len(ref) >= 25 and "--mona_variant" in ref and "--exp" in ref, entry
    for flag, kw in ref.items():
        assert flag in got, (entry, flag)
        if flag != "--device":
            assert got[flag] == kw, (entry, flag, kw, got[flag])


@pytest.mark.parametrize("family,exp,extra", [("clip", "clip_seg", dict(version="ViT-B/16", ckpt="ckpt/ViT-B-16.pt")), ("metaclip", "metaclip_seg", {}),
                                              ("unimedclip", "unimedclip_seg", dict(version="ViT-B-16-quickgelu", ckpt="ckpt/unimed_clip_vit_b16.pt"))])
def test_new_entries_parse_to_the_reference_defaults_and_share_the_supervised_loop(family, exp, extra):
    from src.models import supervised
    mod = importlib.import_module(f"src.models.{family}.segmentation")
    a = mod.get_args([])
    want = dict(exp=exp, dataset="LN-INT", img_size=224, patch_size=16, num_workers=8, strong_augs=True, weak_augs=True, mona_variant="noise_aware",
                mona_weights=None, in_channels=3, num_classes=2, reduce_dim=512, mona_bottleneck=64, mona_layers=None, seed=1, epochs=1000, batch_size=32,
                lr=1e-4, lr_min=1e-8, weight_decay=0.01, beta1=0.9, beta2=0.95, patience=15, test=False, **extra)
    for k, v in want.items():
        assert getattr(a, k) == v, (family, k)
    assert not hasattr(a, "lora_r") and not hasattr(a, "lora_weights")
    assert all(callable(getattr(mod, f)) for f in ("get_args", "prepare_model", "train", "test", "main"))
    t = mod.TASK
    assert t.stop_twice and t.visualize and t.data is supervised.SEGMENTATION.data and t.criterion is supervised.SEGMENTATION.criterion and mod.criterion is t.criterion


# ------------------------------------------------------------------------------------------------ names without samples
def test_name_of_agrees_with_getitem(monkeypatch):
    from src.datasets import classification as C
    from src.datasets import segmentation as S
    syn = S.SyntheticSegmentation(7, 8, seed=3, prefix="test", cache_bytes=0)
    names = [f"d/{i}_x.png" for i in range(5)]
    ten = S.TensorSegmentation(torch.zeros(5, 1, 4, 4), torch.zeros(5, 1, 4, 4), names)
    cls = C.TensorClassification(torch.zeros(5, 1, 4, 4), torch.arange(5) % 2, names)
    for ds in (syn, ten, cls):
        assert len(ds) > 0
        for i in range(len(ds)):
            assert ds.name_of(i) == ds[i][2]
    assert syn.name_of(3) == "test_00003.png"
    made = []
    monkeypatch.setattr(S, "synthetic_sample", lambda *a: made.append(a))
    assert syn.name_of(2) == "test_00002.png" and not made       # the name does not produce the sample


def test_datamodule_test_split_names_in_loader_order():
    from src.datasets import segmentation as S
    args = type("A", (), dict(synthetic=True, data_pt=None, synthetic_train=4, synthetic_val=2, synthetic_test=5, img_size=8, seed=1, batch_size=4, num_workers=0))()
    dm = S.DataModule(args, rank=0, world=1)
    got = [n for batch in dm.test_dataloader() for n in batch[2]]
    assert got == [dm.test_dataset.name_of(i) for i in range(5)]


# ------------------------------------------------------------------------------------------------ --viz
@pytest.mark.parametrize("family", SEG_ENTRIES)
def test_viz_is_on_by_default_and_no_viz_parses(family):
    mod = importlib.import_module(f"src.models.{family}.segmentation")
    assert mod.get_args([]).viz is True
    assert mod.get_args(["--no-viz"]).viz is False and mod.get_args(["--viz"]).viz is True


def test_task_visualize_field():
    from src.models import supervised
    from src.models.clipseg import segmentation as clipseg
    assert supervised.SEGMENTATION.visualize is True and supervised.CLASSIFICATION.visualize is False and clipseg.TASK.visualize is True


# ------------------------------------------------------------------------------------------------ the C entry without a GPU
def test_form_function_is_pure_and_follows_size_and_addresses():
    from uia_hip import _lib
    lib = _lib.lib()
    a = 1 << 20                                                  # any 16-byte aligned address: nothing is dereferenced
    ptrs = [a, 2 * a, 3 * a, 4 * a, 5 * a, 6 * a]
    for S in (4, 8, 64, 224, 352):
        assert lib.uia_seg_viz_form(S, 0, *ptrs) == 1 and lib.uia_seg_viz_form(S, 1, *ptrs) == 1
    for S in (1, 5, 37, 518, 0, -4):
        assert lib.uia_seg_viz_form(S, 0, *ptrs) == 0
    for k in range(6):                                           # one element into its buffer: 4 bytes for an fp32 input, 1 for the bytes
        for code in (0, 1):
            p = list(ptrs)
            p[k] += 4 if (k < 2 or (k == 2 and code == 1)) else 1
            assert lib.uia_seg_viz_form(64, code, *p) == 0, (k, code)
    p = list(ptrs)
    p[2] += 4                                                    # uint8 labels need 4 bytes only, fp32 labels 16
    assert lib.uia_seg_viz_form(64, 0, *p) == 1 and lib.uia_seg_viz_form(64, 1, *p) == 0


def test_entry_refuses_bad_arguments_before_touching_a_device():
    from uia_hip import _lib
    lib = _lib.lib()
    a = 1 << 24
    lg, im, lb, m, o, p = (a * k for k in range(1, 7))
    ok = dict(B=2, C=2, Ci=3, S=8, lg=lg, im=im, lb=lb, code=0, m=m, o=o, p=p)

    def call(**kw):
        v = dict(ok, **kw)
        return lib.uia_seg_viz(None, v["B"], v["C"], v["Ci"], v["S"], v["lg"], v["im"], v["lb"], v["code"], v["m"], v["o"], v["p"])

    for kw, word in ((dict(lg=None), "null"), (dict(im=None), "null"), (dict(lb=None), "null"), (dict(m=None), "null"), (dict(o=None), "null"),
                     (dict(p=None), "null"), (dict(B=0), "bad shape"), (dict(B=-1), "bad shape"), (dict(S=0), "bad shape"), (dict(S=-8), "bad shape"),
                     (dict(C=1), "classes"), (dict(C=3), "classes"), (dict(Ci=2), "channels"), (dict(Ci=0), "channels"), (dict(Ci=4), "channels"),
                     (dict(code=2), "label dtype"), (dict(code=-1), "label dtype"), (dict(o=m), "overlaps"), (dict(o=m + 8 * 8 * 2 * 3 - 1), "overlaps"),
                     (dict(p=m + 5), "overlaps"), (dict(p=o), "overlaps"), (dict(m=lg + 16), "overlaps"), (dict(o=im), "overlaps"), (dict(p=lb + 127), "overlaps"),
                     (dict(lg=lg + 2), "4-byte")):
        assert call(**kw) != 0, kw
        assert word in lib.uia_last_error().decode(), (kw, lib.uia_last_error().decode())


def test_new_export_is_declared_typed_and_wrapped():
    from uia_hip import _lib, ops
    header = open(os.path.join(ROOT, "include", "uia_hip.h")).read()
    for name in ("uia_seg_viz", "uia_seg_viz_form"):
        assert name + "(" in header and name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    with pytest.raises(_lib.UiaError):
        ops.seg_viz(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4, dtype=torch.uint8))


def test_product_path_does_not_import_pil_or_the_oracle():
    import subprocess
    code = ("import sys; sys.path[:0] = [%r, %r]; import src.utils.viz, src.utils.tools, src.models.supervised, src.models.clip.segmentation, "
            "src.models.metaclip.segmentation, src.models.unimedclip.segmentation; bad = [m for m in sys.modules if m == 'PIL' or m.startswith(('PIL.', 'oracle'))]; "
            "assert not bad, bad" % (ROOT, os.path.join(ROOT, "nextgen-uia_amd")))
    subprocess.run([sys.executable, "-c", code], check=True)
