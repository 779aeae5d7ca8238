"""-m gpu: src/models/predict.py end to end on the two smallest real entries.  A child process trains the baseline for one epoch on synthetic data at
img_size 32, a fresh child process predicts on six pictures of different sizes written here with Pillow, and the files are held against the pictures and
against an in-process run of the same model, checkpoint and uia_hip.ops.seg_predict_native."""
import csv
import os
import subprocess
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

pytestmark = pytest.mark.gpu
S, BATCH = 32, 4
SIZES = {"a_wide.png": (100, 75), "b_thin.png": (40, 3), "c_tall.png": (33, 47), "d_photo.jpg": (57, 21), "e_square.png": (64, 64), "f_same.png": (32, 32)}   # (W, H)
FLAGS = ["--img_size", str(S), "--batch_size", str(BATCH), "--num_workers", "0"]
TRAIN = ["--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4", "--epochs", "1", "--no-viz"]
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))


def child(cmd, cwd, timeout):
    r = subprocess.run([sys.executable, "-m"] + cmd, cwd=cwd, env=ENV, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """A working directory with the six pictures and one trained checkpoint per baseline entry."""
    d = tmp_path_factory.mktemp("predict")
    (d / "pics").mkdir()
    rng = np.random.default_rng(0)
    for name, (W, H) in SIZES.items():
        Image.fromarray(rng.integers(0, 256, size=(H, W), dtype=np.uint8)).save(d / "pics" / name)
    for kind, exp in (("segmentation", "ps"), ("classification", "pc")):
        child([f"src.models.baselines.{kind}", "--exp", exp] + FLAGS + TRAIN, d, 300)
        assert os.path.isfile(d / "runs" / exp / "LN-INT" / "train" / "best_model.pth")
    return d


def predict(work, kind, exp, out, extra=()):
    return child(["src.models.predict", "--entry", f"baselines.{kind}", "--images", "pics", "--out", out, *extra, "--", "--exp", exp] + FLAGS, work, 300)


def in_process(work, kind, exp):
    """-> per batch (names, RaggedBatch on the device, logits): the entry's model with the child's checkpoint, on the pictures decoded here."""
    import importlib
    from src.datasets import folder
    from src.datasets.image_dir import ImageDir, ImageDirCollate
    from src.models import predict as P, supervised
    from uia_hip import functional as UF
    module = importlib.import_module(f"src.models.baselines.{kind}")
    args = module.get_args(["--exp", exp] + FLAGS)
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model = P.load_model(module, args, str(work / "runs" / exp / "LN-INT" / "train" / "best_model.pth"))
    task = supervised.SEGMENTATION if kind == "segmentation" else supervised.CLASSIFICATION
    ds = ImageDir(str(work / "pics"), S)
    resize = folder.ResizeStage(S, with_mask=kind == "segmentation")
    out = []
    with torch.no_grad():
        for at in range(0, len(ds), BATCH):
            buf, desc, _, (names, _) = ImageDirCollate(S)([ds[i] for i in range(at, min(at + BATCH, len(ds)))])
            batch = folder.RaggedBatch(buf.to("cuda:0"), desc)
            images, second = resize(batch, None)
            images, _ = task.to_input(images, second, args.in_channels)
            out.append((names, batch, model(images).detach().float().clone()))
    return out


def test_segmentation_masks_overlays_and_csv(work):
    from src.utils.viz import NativeMaskWriter
    from uia_hip import ops
    r = predict(work, "segmentation", "ps", "out_seg")
    assert '"images": 6' in r.stdout
    out = work / "out_seg"
    names = sorted(SIZES)
    assert sorted(os.listdir(out)) == ["masks", "overlays", "predictions.csv"]
    stems = [os.path.splitext(n)[0] for n in names]
    assert sorted(os.listdir(out / "masks")) == [s + ".png" for s in stems] and sorted(os.listdir(out / "overlays")) == [s + ".png" for s in stems]
    rows = list(csv.reader(open(out / "predictions.csv")))
    assert rows[0] == "name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax".split(",")
    assert [r[0] for r in rows[1:]] == names                     # the six rows, in name order
    masks = {}
    for name, stem, row in zip(names, stems, rows[1:]):
        W, H = SIZES[name]
        m, o = Image.open(out / "masks" / f"{stem}.png"), Image.open(out / "overlays" / f"{stem}.png")
        assert (m.mode, m.size, o.mode, o.size) == ("L", (W, H), "RGB", (W, H)), name
        mask, over = np.asarray(m), np.asarray(o)
        masks[name] = mask
        assert set(np.unique(mask)) <= {0, 255}
        g = np.asarray(Image.open(work / "pics" / name).convert("L"))
        assert np.array_equal(over, np.stack([g, np.maximum(g, mask), g], axis=-1)), name
        n = int((mask > 0).sum())
        assert (int(row[1]), int(row[2]), int(row[3])) == (W, H, n) and row[4] == f"{n / (W * H):.6f}", (name, row)
        ys, xs = np.nonzero(mask)
        assert row[5:] == ([str(ys.min()), str(xs.min()), str(ys.max()), str(xs.max())] if n else ["", "", "", ""]), (name, row)
    # the same model, checkpoint and launch in this process give the same bytes
    for batch_names, batch, logits in in_process(work, "segmentation", "ps"):
        sizes = [(H, W) for _, H, W in batch.desc[:, :3].tolist()]
        where, total = NativeMaskWriter.layout(sizes, overlay=False)
        desc = torch.tensor([[-1, H, W, moff, -1, 0, 0, 0] for (H, W), (moff, _) in zip(sizes, where)], dtype=torch.int32)
        flat = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        ops.seg_predict_native(logits, None, desc, flat)
        flat = flat.cpu().numpy()
        for name, (H, W), (moff, _) in zip(batch_names, sizes, where):
            assert np.array_equal(flat[moff:moff + H * W].reshape(H, W), masks[name]), name


def test_no_overlay_writes_no_overlay_folder(work):
    predict(work, "segmentation", "ps", "out_plain", ["--no-overlay"])
    assert sorted(os.listdir(work / "out_plain")) == ["masks", "predictions.csv"]
    assert len(os.listdir(work / "out_plain" / "masks")) == 6
    if os.path.isdir(work / "out_seg"):                          # the masks do not depend on the overlay
        for f in os.listdir(work / "out_plain" / "masks"):
            assert open(work / "out_plain" / "masks" / f, "rb").read() == open(work / "out_seg" / "masks" / f, "rb").read()


def test_classification_csv(work):
    from src.models import predict as P
    predict(work, "classification", "pc", "out_cls")
    assert os.listdir(work / "out_cls") == ["predictions.csv"]
    text = open(work / "out_cls" / "predictions.csv").read()
    rows = list(csv.reader(text.splitlines()))
    names = sorted(SIZES)
    assert rows[0] == "name,width,height,p0,p1,predicted".split(",") and [r[0] for r in rows[1:]] == names
    for name, row in zip(names, rows[1:]):
        p0, p1 = float(row[3]), float(row[4])
        assert (int(row[1]), int(row[2])) == SIZES[name] and abs(p0 + p1 - 1.0) <= 1e-6 and int(row[5]) == (1 if p1 > p0 else 0), row
    probs = torch.cat([torch.softmax(logits, dim=1) for _, _, logits in in_process(work, "classification", "pc")]).cpu().tolist()
    assert text == P.cls_csv(names, [(H, W) for W, H in (SIZES[n] for n in names)], probs)
