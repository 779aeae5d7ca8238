"""-m gpu: the ensemble flags of src/models/predict.py end to end on the two smallest real entries, after tests/test_predict_gpu.py.  A child process trains
the baseline for one epoch on synthetic data at img_size 32; a fresh child process predicts on six pictures of different sizes with two checkpoints (the
same file twice) x four flips = 8 members, a threshold, both maps and the component filter; the files are held against the pictures, against an in-process
run of the same model, checkpoint and uia_hip.ops.seg_predict_native_ens, and against predictions.csv.  A run without any new flag must write what it
wrote before the flags existed."""
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
OLD_HEADER = "name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax"
FLIPS = [0, 1, 2, 3]
THRESHOLD, MIN_AREA = 0.4, 5


def child(cmd, cwd, timeout):
    r = subprocess.run([sys.executable, "-m"] + cmd, cwd=cwd, env=ENV, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def checkpoint(work, exp):
    return work / "runs" / exp / "LN-INT" / "train" / "best_model.pth"


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """A working directory with the six pictures and one trained checkpoint per baseline entry."""
    d = tmp_path_factory.mktemp("predict_ens")
    (d / "pics").mkdir()
    rng = np.random.default_rng(0)
    for name, (W, H) in SIZES.items():
        Image.fromarray(rng.integers(0, 256, size=(H, W), dtype=np.uint8)).save(d / "pics" / name)
    for kind, exp in (("segmentation", "ps"), ("classification", "pc")):
        child([f"src.models.baselines.{kind}", "--exp", exp] + FLAGS + TRAIN, d, 300)
        assert os.path.isfile(checkpoint(d, exp))
    return d


def predict(work, kind, exp, out, extra=()):
    return child(["src.models.predict", "--entry", f"baselines.{kind}", "--images", "pics", "--out", out, *extra, "--", "--exp", exp] + FLAGS, work, 300)


def in_process(work, kind, exp):
    """-> (model, per batch (names, RaggedBatch on the device, the model's S x S input)): the entry's model with the child's checkpoint, on the pictures
    decoded here."""
    import importlib
    from src.datasets import folder
    from src.datasets.image_dir import ImageDir, ImageDirCollate
    from src.models import predict as P, supervised
    from uia_hip import functional as UF
    module = importlib.import_module(f"src.models.baselines.{kind}")
    args = module.get_args(["--exp", exp] + FLAGS)
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model = P.load_model(module, args, str(checkpoint(work, exp)))
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
            out.append((names, batch, images.clone()))
    return model, out


def flipped(images, f):
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if f & bit]
    return torch.flip(images, dims) if dims else images


def test_eight_members_with_maps_threshold_and_filter(work):
    from src.utils.viz import NativeMaskWriter
    from uia_hip import ops
    ck = str(checkpoint(work, "ps"))
    r = predict(work, "segmentation", "ps", "out_ens", ["--ensemble", ck, "--tta", "flips", "--prob", "--spread", "--threshold", str(THRESHOLD), "--min_area",
                                                         str(MIN_AREA)])
    assert '"images": 6' in r.stdout
    out = work / "out_ens"
    names = sorted(SIZES)
    stems = [os.path.splitext(n)[0] for n in names]
    folders = ["masks", "overlays", "probs", "spread"]
    assert sorted(os.listdir(out)) == sorted(folders + ["predictions.csv"])
    files = {}
    for folder in folders:
        assert sorted(os.listdir(out / folder)) == [s + ".png" for s in stems], folder
        for name, stem in zip(names, stems):
            im = Image.open(out / folder / f"{stem}.png")
            assert (im.mode, im.size) == ("RGB" if folder == "overlays" else "L", SIZES[name]), (folder, name)
            files[folder, name] = np.asarray(im)
    for name in names:
        mask = files["masks", name]
        g = np.asarray(Image.open(work / "pics" / name).convert("L"))
        assert set(np.unique(mask)) <= {0, 255}
        assert np.array_equal(files["overlays", name], np.stack([g, np.maximum(g, mask), g], axis=-1)), name

    # the same model, checkpoint, launch and filter in this process give the same bytes; two checkpoints that are one file are the same four members twice
    model, batches = in_process(work, "segmentation", "ps")
    unfiltered = {}
    with torch.no_grad():
        for batch_names, batch, images in batches:
            four = [model(flipped(images, f)).detach().float() for f in FLIPS]
            stack = torch.stack(four + four).contiguous()
            sizes = [(H, W) for _, H, W in batch.desc[:, :3].tolist()]
            where, total = NativeMaskWriter.layout(sizes, overlay=False, prob=True, spread=True)
            desc = torch.tensor([[-1, H, W, moff, -1, poff, roff, 0] for (H, W), (moff, _, poff, roff) in zip(sizes, where)], dtype=torch.int32)
            flat = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
            stats, sums = ops.seg_predict_native_ens(stack, FLIPS + FLIPS, None, desc, flat, threshold=THRESHOLD)
            before, stats, sums = flat.cpu().numpy(), stats.cpu().numpy(), sums.cpu().numpy()
            cdesc = torch.tensor([[moff, H, W, -1, MIN_AREA, 0, 8, 0] for (H, W), (moff, _, _, _) in zip(sizes, where)], dtype=torch.int32)
            ops.mask_components(flat, cdesc)
            after = flat.cpu().numpy()
            for i, (name, (H, W), (moff, _, poff, roff)) in enumerate(zip(batch_names, sizes, where)):
                assert np.array_equal(after[moff:moff + H * W].reshape(H, W), files["masks", name]), name
                assert np.array_equal(after[poff:poff + H * W].reshape(H, W), files["probs", name]), name
                assert np.array_equal(after[roff:roff + H * W].reshape(H, W), files["spread", name]), name
                unfiltered[name] = before[moff:moff + H * W].reshape(H, W)
                assert int(stats[i, 0]) == int((unfiltered[name] == 255).sum()) and int(sums[i, 1]) == int(files["spread", name].astype(np.int64).sum())
    assert any(files["spread", n].any() for n in names) and any(files["probs", n].min() < files["probs", n].max() for n in names)

    # predictions.csv: the old columns describe the filtered mask file, the two new ones the maps
    rows = list(csv.reader(open(out / "predictions.csv")))
    assert rows[0] == (OLD_HEADER + ",mean_foreground_probability,mean_spread").split(",") and [r[0] for r in rows[1:]] == names
    for name, row in zip(names, rows[1:]):
        W, H = SIZES[name]
        mask, q, spread = files["masks", name], files["probs", name], files["spread", name]
        n = int((mask > 0).sum())
        assert (int(row[1]), int(row[2]), int(row[3])) == (W, H, n) and row[4] == f"{n / (W * H):.6f}", (name, row)
        ys, xs = np.nonzero(mask)
        assert row[5:9] == ([str(ys.min()), str(xs.min()), str(ys.max()), str(xs.max())] if n else ["", "", "", ""]), (name, row)
        fg = unfiltered[name] == 255
        assert n <= int(fg.sum())
        assert row[9] == (f"{int(q[fg].astype(np.int64).sum()) / (255 * int(fg.sum())):.6f}" if fg.any() else ""), (name, row)
        assert row[10] == f"{int(spread.astype(np.int64).sum()) / (255 * W * H):.6f}", (name, row)
        assert len(row) == 11


def test_without_the_new_flags_the_files_are_what_they_were(work):
    """The path of tests/test_predict_gpu.py: one checkpoint, uia_seg_predict_native, the old header — the files byte for byte."""
    from src.models import predict as P
    from src.utils.viz import NativeMaskWriter, encode_png
    from uia_hip import ops
    predict(work, "segmentation", "ps", "out_plain")
    out = work / "out_plain"
    assert sorted(os.listdir(out)) == ["masks", "overlays", "predictions.csv"]
    model, batches = in_process(work, "segmentation", "ps")
    all_names, all_sizes, all_stats = [], [], []
    with torch.no_grad():
        for batch_names, batch, images in batches:
            logits = model(images).detach().float()
            geo = batch.desc[:, :3].tolist()
            sizes = [(H, W) for _, H, W in geo]
            where, total = NativeMaskWriter.layout(sizes, overlay=True)
            desc = torch.tensor([[off, H, W, moff, ooff, 0, 0, 0] for (off, H, W), (moff, ooff) in zip(geo, where)], dtype=torch.int32)
            flat = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
            stats = ops.seg_predict_native(logits, batch.data, desc, flat)
            flat = flat.cpu().numpy()
            for name, (H, W), (moff, ooff) in zip(batch_names, sizes, where):
                stem = os.path.splitext(name)[0]
                assert open(out / "masks" / f"{stem}.png", "rb").read() == encode_png(flat[moff:moff + H * W].reshape(H, W)), name
                assert open(out / "overlays" / f"{stem}.png", "rb").read() == encode_png(flat[ooff:ooff + 3 * H * W].reshape(H, W, 3)), name
            all_names += batch_names
            all_sizes += sizes
            all_stats += stats.cpu().tolist()
    text = open(out / "predictions.csv").read()
    assert text.splitlines()[0] == OLD_HEADER and text == P.seg_csv(all_names, all_sizes, all_stats)


def test_classification_averages_the_softmax_of_the_flips(work):
    from src.models import predict as P
    predict(work, "classification", "pc", "out_cls_tta", ["--tta", "hflip"])
    assert os.listdir(work / "out_cls_tta") == ["predictions.csv"]
    text = open(work / "out_cls_tta" / "predictions.csv").read()
    names = sorted(SIZES)
    model, batches = in_process(work, "classification", "pc")
    probs = []
    with torch.no_grad():
        for _, _, images in batches:
            stack = torch.stack([model(flipped(images, f)).detach().float() for f in (0, 1)])
            probs.append(torch.softmax(stack, dim=2).mean(dim=0))
        plain = [torch.softmax(model(images).detach().float(), dim=1) for _, _, images in batches]
    probs = torch.cat(probs).cpu().tolist()
    assert text.splitlines()[0] == "name,width,height,p0,p1,predicted"
    assert text == P.cls_csv(names, [(H, W) for W, H in (SIZES[n] for n in names)], probs)
    assert text !=P.cls_csv(names, [(H, W) for W, H in (SIZES[n] for n in names)], torch.cat(plain).cpu().tolist())      # the flip member counts
