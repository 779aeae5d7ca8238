"""-m gpu: uia_mask_morphology (csrc/morphology.hip) against tests/morphology_reference.py (shifted-mask dilation, complement erosion, explicit-stack
flood fill: nothing of the kernel's formulation), exactly: every mask byte, every overlay byte, all eight stats words, and the sentinel bytes and words
round them.  Then NativeMaskWriter's three arguments and the command line's three flags, against the same reference and an in-process run."""
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

import morphology_reference as R  # noqa: E402

Image = pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BYTE, SENT_WORD = 0xA5, 0x5EA7BEEF
SMALL = [(1, 1), (1, 37), (37, 1), (7, 5), (33, 65), (65, 33), (130, 70), (70, 130)]
RADII = (1, 2, 3, 5, 17, 64)
# (r_close, r_open, hole_area, hole_connectivity): each radius alone, four mixed pairs, every hole_area under both connectivities, the identity, and
# closing + fill + opening together.  Radii above 5 cost the yardstick most (12 853 shifted copies at 64), so they meet the contents of WIDE only.
CHEAP = ([(r, 0, 0, 4) for r in RADII if r <= 5] + [(0, r, 0, 8) for r in RADII if r <= 5] + [(1, 1, 0, 4), (3, 2, 0, 8)]
         + [(0, 0, a, c) for a in (-1, 1, 5, 50) for c in (4, 8)] + [(0, 0, 0, 4), (0, 0, 0, 8), (1, 0, -1, 4), (1, 0, -1, 8), (2, 1, -1, 4), (3, 2, 50, 8), (5, 1, 5, 4)])
DEAR = [(17, 0, 0, 4), (64, 0, 0, 8), (0, 17, 0, 8), (0, 64, 0, 4), (5, 17, -1, 4), (64, 3, -1, 8)]
WIDE = ("empty", "full", "one_pixel", "noise0.3", "noise0.7", "bridge", "blob_on_frame")


def lay_out(images, start):
    """images: [(mask, overlay or None, (r_close, r_open, hole_area, hole_connectivity))] -> (host buffer with sentinel bytes before, between and after
    the ranges, desc int32 [B, 8], [(mask offset, overlay offset)]).  Gaps of 1 .. 3 bytes keep the offsets of every alignment."""
    at, where, parts = start, [], [np.full(start, SENT_BYTE, np.uint8)]
    for k, (mask, over, _) in enumerate(images):
        moff, at = at, at + mask.size
        gap = 1 + k % 3
        parts += [mask.ravel(), np.full(gap, SENT_BYTE, np.uint8)]
        at += gap
        ooff = -1
        if over is not None:
            ooff, at = at, at + over.size
            parts += [over.ravel(), np.full(gap, SENT_BYTE, np.uint8)]
            at += gap
        where.append((moff, ooff))
    desc = np.array([[moff, *mask.shape, ooff, *p] for (mask, _, p), (moff, ooff) in zip(images, where)], dtype=np.int32)
    return np.concatenate(parts), desc, where


def launch(buf, desc):
    """One call of the C entry on the device buffer `buf` with stats inside a larger tensor of sentinel words -> stats on the host."""
    from uia_hip import _lib, ops
    B = desc.shape[0]
    stats = torch.full((8 + B * 8 + 8,), SENT_WORD, dtype=torch.int32, device=DEV)
    ws = ops.mask_morphology_workspace(B, int((desc[:, 1].astype(np.int64) * desc[:, 2]).sum()), torch.device(DEV))
    hdesc = torch.from_numpy(np.ascontiguousarray(desc))
    rc = _lib.lib().uia_mask_morphology(torch.cuda.current_stream().cuda_stream, B, buf.data_ptr(), buf.numel(), hdesc.data_ptr(), ws.data_ptr(), ws.numel(),
                                        stats[8:].data_ptr())
    assert rc == 0, _lib.lib().uia_last_error().decode()
    torch.cuda.synchronize()
    stats = stats.cpu().numpy()
    assert (stats[:8] == SENT_WORD).all() and (stats[-8:] == SENT_WORD).all(), "a word beside stats was written"
    return stats[8:-8].reshape(B, 8)


def expected(images, where, host):
    want, stats = host.copy(), []
    for (mask, over, (rc, ro, area, conn)), (moff, ooff) in zip(images, where):
        m, o, s = R.apply(mask, over, rc, ro, area, conn)
        want[moff:moff + m.size] = m.ravel()
        if o is not None:
            want[ooff:ooff + o.size] = o.ravel()
        stats.append(s)
    return want, np.stack(stats)


def run_and_compare(images, start=1, names=None):
    host, desc, where = lay_out(images, start)
    buf = torch.from_numpy(host).to(DEV)
    stats = launch(buf, desc)
    got = buf.cpu().numpy()
    want, wstats = expected(images, where, host)
    for k, (mask, over, p) in enumerate(images):
        what = f"image {k} ({names[k] if names else ''}): {mask.shape}, overlay={over is not None}, (r_close, r_open, hole_area, connectivity)={p}"
        assert np.array_equal(stats[k], wstats[k]), (what, stats[k].tolist(), wstats[k].tolist())
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        k = max(i for i, (moff, _) in enumerate(where) if moff <= at)
        raise AssertionError(f"byte {at} of the buffer is {got[at]}, expected {want[at]} (was {host[at]}); image {k} {names[k] if names else ''} at {where[k]}, "
                             f"{images[k][0].shape}, {images[k][2]}")
    return buf, desc, stats, host, want, wstats


def grid_images(H, W, names, params):
    pats, out, tags = R.patterns(H, W), [], []
    for name in names:
        for p in params:
            m = pats[name]
            out.append((m, R.overlay_of(m, len(out)) if len(out) % 2 == 0 else None, p))
            tags.append(name)
    return out, tags


# ------------------------------------------------------------------------------------------------ the main sweep
@pytest.mark.parametrize("part", ["radii_to_5_and_fills", "radii_17_and_64"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_content_and_setting(shape, part):
    """One image per (content, setting) in ONE call: a ragged batch at an odd offset, every other image with an overlay; radii beyond the image included.
    (Two cases per size only because the yardstick, not the kernel, needs seconds for them.)"""
    H, W = shape
    images, tags = grid_images(H, W, sorted(R.patterns(H, W)), CHEAP) if part == "radii_to_5_and_fills" else grid_images(H, W, WIDE, DEAR)
    run_and_compare(images, start=1, names=tags)


def test_several_tiles_both_ways():
    """300 x 517: ten tile rows, nine tile columns, neither a multiple of the tile; the seam-heavy contents; radii up to 17."""
    H, W = 300, 517
    pats = R.patterns(H, W)
    settings = {"checkerboard": [(1, 0, -1, 4), (0, 1, 0, 8)], "noise0.5": [(0, 0, -1, 4), (0, 0, 5, 8), (2, 1, -1, 4)], "noise0.3": [(3, 0, 50, 8), (17, 0, -1, 4)],
                "noise0.7": [(0, 2, -1, 8), (0, 17, 0, 4)], "ring_in_ring": [(0, 0, -1, 4), (5, 3, -1, 8)], "ring_diagonal_gap": [(0, 0, -1, 4), (0, 0, -1, 8)],
                "ring_gap5": [(5, 0, -1, 4), (17, 5, -1, 8)], "bridge": [(0, 2, 0, 4)]}
    images, tags = [], []
    for name, ps in settings.items():
        for p in ps:
            images.append((pats[name], R.overlay_of(pats[name], 3) if len(images) % 3 == 0 else None, p))
            tags.append(name)
    run_and_compare(images, start=3, names=tags)


def test_a_hole_through_several_hundred_tiles():
    """16384 x 64: 512 tiles in one column.  A channel one pixel wide runs down the middle of a solid bar and ends inside it: one hole of 16000 pixels whose
    root every tile must reach; a second channel reaches the last row and is none."""
    H, W = 16384, 64
    m = np.zeros((H, W), dtype=np.uint8)
    m[100:H, :] = 255
    m[200:16200, 20] = 0                              # the hole
    m[300:H, 40] = 0                                  # open at the frame
    m[5:40:7, 3:60:5] = 255                           # speckle for the opening
    for p, filled in (((0, 0, -1, 4), 16000), ((0, 3, -1, 8), None), ((3, 0, 0, 4), None)):
        _, _, stats, _, _, wstats = run_and_compare([(m, None, p)], start=5)
        if filled is not None:
            assert stats[0, 5] == filled and stats[0, 6] == 0


def test_a_batch_that_mixes_images_with_and_without_each_operation():
    shapes = [(33, 65), (70, 130), (7, 5), (65, 33), (130, 70), (1, 37), (40, 200), (64, 64)]
    params = [(0, 0, 0, 4), (2, 0, 0, 4), (0, 0, -1, 8), (0, 3, 0, 8), (2, 0, -1, 4), (0, 1, 5, 4), (5, 2, 0, 8), (3, 2, -1, 4)]
    images = []
    for k, ((H, W), p) in enumerate(zip(shapes, params)):
        m = R.patterns(H, W)[("noise0.5", "ring_gap2", "noise0.3", "values")[k % 4]]
        images.append((m, R.overlay_of(m, k) if k % 2 else None, p))
    run_and_compare(images, start=7)
    run_and_compare(images[::-1], start=2)
    run_and_compare([(m, None, p) for m, _, p in images], start=1)             # no overlay at all
    run_and_compare([(m, R.overlay_of(m, 1), p) for m, _, p in images], start=1)


def test_two_calls_agree_and_the_single_operations_are_idempotent():
    H, W = 130, 70
    pats = R.patterns(H, W)
    images = [(pats[n], R.overlay_of(pats[n], k), p) for k, (n, p) in enumerate([("noise0.3", (3, 0, 0, 4)), ("noise0.7", (0, 2, 0, 8)), ("noise0.5", (0, 0, -1, 4)),
                                                                               ("ring_gap1", (1, 0, 0, 4)), ("bridge", (0, 5, 0, 4)), ("ring_in_ring", (0, 0, 50, 8))])]
    buf, desc, stats, host, want, _ = run_and_compare(images, start=1)
    again = torch.from_numpy(host).to(DEV)
    stats2 = launch(again, desc)
    assert np.array_equal(again.cpu().numpy(), want) and np.array_equal(stats, stats2)
    # r_close alone never removes, r_open alone never adds
    assert (stats[[0, 3], 6] == 0).all() and (stats[[1, 4], 5] == 0).all() and stats[:, 5:7].sum() > 0
    # a second call with the same single operation changes nothing and reports added = removed = 0
    stats3 = launch(buf, desc)
    assert np.array_equal(buf.cpu().numpy(), want)
    assert (stats3[:, 5:7] == 0).all() and np.array_equal(stats3[:, :5], stats[:, :5]) and np.array_equal(stats3[:, 7], stats[:, 0])


def test_the_wrapper_returns_what_the_entry_writes():
    from uia_hip import ops
    images, _ = grid_images(33, 65, ("noise0.5", "ring_gap2"), [(1, 1, -1, 4), (0, 0, 0, 8)])
    host, desc, where = lay_out(images, 1)
    buf = torch.from_numpy(host).to(DEV)
    stats = ops.mask_morphology(buf, torch.from_numpy(desc))
    want, wstats = expected(images, where, host)
    assert stats.dtype == torch.int32 and tuple(stats.shape) == (4, 8) and stats.is_cuda
    assert np.array_equal(stats.cpu().numpy(), wstats) and np.array_equal(buf.cpu().numpy(), want)
    assert ops.MASK_MORPHOLOGY_DESC == 8 and ops.MORPHOLOGY_MAX_RADIUS == 64


def test_one_call_per_refusal_leaves_the_device_untouched():
    from uia_hip import ops
    from uia_hip.ops import UiaError
    m = R.patterns(7, 5)["noise0.5"]
    host, desc, _ = lay_out([(m, R.overlay_of(m), (1, 1, -1, 4)), (m, None, (0, 0, 0, 8))], 1)

    def edit(b, w, v):
        d = desc.copy()
        d[b, w] = v
        return d
    cases = [(edit(0, 4, 65), "r_close 65"), (edit(1, 5, -1), "r_open -1"), (edit(0, 6, -2), "hole_area -2"), (edit(1, 7, 6), "hole_connectivity 6"),
             (edit(0, 1, 0), "image 0 is 0 x 5"), (edit(1, 2, 16385), "image 1 is 7 x 16385"), (edit(0, 0, -1), "the mask of image 0"),
             (edit(0, 3, -2), "overlay offset -2"), (edit(1, 0, len(host) - 10), "the mask of image 1"), (edit(1, 0, 3), "overlaps"),
             (edit(0, 3, len(host) - 20), "the overlay of image 0")]
    for d, word in cases:
        buf = torch.from_numpy(host).to(DEV)
        with pytest.raises(UiaError, match=word):
            ops.mask_morphology(buf, torch.from_numpy(d))
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), host), word
    buf = torch.from_numpy(host).to(DEV)
    for bad_buf, bad_desc in ((buf.cpu(), desc), (buf.view(-1, 1), desc), (buf.int(), desc), (buf, desc.astype(np.int64)), (buf, desc[:, :7].copy()), (buf, desc[:0])):
        with pytest.raises(UiaError, match="mask_morphology"):
            ops.mask_morphology(bad_buf, torch.from_numpy(np.ascontiguousarray(bad_desc)))
    with pytest.raises(UiaError, match="mask_morphology"):
        ops.mask_morphology(buf, torch.from_numpy(desc).to(DEV))


# ------------------------------------------------------------------------------------------------ NativeMaskWriter
WRITER_S = 32
WRITER_SIZES = [(75, 100), (47, 33), (64, 64), (21, 57)]          # (H, W)


def synthetic_batch():
    """Four gray pictures of different sizes as a folder.RaggedBatch on the device, and logits whose arg-max has blobs, holes and speckle."""
    from src.datasets import folder
    rng = np.random.default_rng(11)
    pics = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in WRITER_SIZES]
    at, rows = 0, []
    for H, W in WRITER_SIZES:
        rows.append([at, H, W, -1, WRITER_S, WRITER_S, 0, 0])
        at += H * W
    data = torch.from_numpy(np.concatenate([p.ravel() for p in pics])).to(DEV)
    g = torch.Generator().manual_seed(5)
    coarse = torch.nn.functional.interpolate(torch.randn(4, 1, 6, 6, generator=g), size=(WRITER_S, WRITER_S), mode="bilinear", align_corners=False)
    diff = coarse + 0.35 * torch.randn(4, 1, WRITER_S, WRITER_S, generator=g)
    logits = torch.cat([torch.zeros_like(diff), diff], dim=1).contiguous().to(DEV)
    return folder.RaggedBatch(data, torch.tensor(rows, dtype=torch.int32)), logits, pics, [f"p{k}.png" for k in range(4)]


def files_of(d):
    return {os.path.join(sub, f): open(os.path.join(d, sub, f), "rb").read() for sub in ("masks", "overlays") for f in sorted(os.listdir(os.path.join(d, sub)))}


def test_writer_with_and_without_the_arguments(tmp_path, monkeypatch):
    import components_reference as CR
    from src.utils import viz
    from uia_hip import ops
    batch, logits, pics, names = synthetic_batch()

    def write(out, **kw):
        w = viz.NativeMaskWriter(tmp_path / out, overlay=True, **kw)
        w.submit(logits, batch, names)
        return w.close(), w.morphology_stats(), w.lesion_lists()

    real = ops.mask_morphology
    monkeypatch.setattr(ops, "mask_morphology", lambda *a, **k: (_ for _ in ()).throw(AssertionError("mask_morphology was called with the defaults")))
    (plain,), none, _ = write("plain")
    (explicit,), none2, _ = write("explicit", close_radius=0, open_radius=0, fill_holes=0)
    monkeypatch.setattr(ops, "mask_morphology", real)
    assert none == [] and none2 == [] and np.array_equal(plain[2], explicit[2])

    # without the arguments: byte for byte what seg_predict_native alone gives
    where, total = viz.NativeMaskWriter.layout(WRITER_SIZES, True)
    desc = torch.tensor([[off, H, W, moff, ooff, 0, 0, 0] for (off, H, W), (moff, ooff) in zip(batch.desc[:, :3].tolist(), where)], dtype=torch.int32)
    flat = torch.zeros(total, dtype=torch.uint8, device=DEV)
    native = ops.seg_predict_native(logits, batch.data, desc, flat).cpu().numpy()
    flat = flat.cpu().numpy()
    want = {}
    for name, (H, W), (moff, ooff) in zip(names, WRITER_SIZES, where):
        want[os.path.join("masks", name)] = viz.encode_png(flat[moff:moff + H * W].reshape(H, W))
        want[os.path.join("overlays", name)] = viz.encode_png(flat[ooff:ooff + 3 * H * W].reshape(H, W, 3))
    assert files_of(tmp_path / "plain") == want and files_of(tmp_path / "explicit") == want and np.array_equal(plain[2], native)

    # with them: the morphology call, then the component call on its result; connectivity 8 -> holes joined by 4, and the other way round
    changed = 0
    for out, conn in (("morph8", 8), ("morph4", 4)):
        (done,), (morph,), (lists,) = write(out, close_radius=2, open_radius=1, fill_holes=-1, min_area=20, connectivity=conn, lesions=2)
        assert morph.shape == (4, 3) and morph.dtype == np.int32 and lists.shape == (4, 2, 8)
        got = files_of(tmp_path / out)
        for k, (name, (H, W), (moff, ooff)) in enumerate(zip(names, WRITER_SIZES, where)):
            mask, over = flat[moff:moff + H * W].reshape(H, W), flat[ooff:ooff + 3 * H * W].reshape(H, W, 3)
            m, o, s = R.apply(mask, over, 2, 1, -1, 12 - conn)
            assert morph[k].tolist() == [int(s[5]), int(s[6]), int(native[k][0])], (name, morph[k], s)
            changed += int(s[5]) + int(s[6])
            m, o, cs, rows = CR.apply(m, o, min_area=20, keep=0, connectivity=conn, max_list=2)
            assert got[os.path.join("masks", name)] == viz.encode_png(m) and got[os.path.join("overlays", name)] == viz.encode_png(o), (out, name)
            assert np.array_equal(done[2][k], cs) and np.array_equal(lists[k], rows), (out, name, done[2][k], cs)
    assert changed > 0, "the synthetic logits must give the morphology something to do"
    # the morphology alone: the slot's stats are the call's own
    (done,), (morph,), lists = write("alone", fill_holes=5)
    assert lists == []
    for k, ((H, W), (moff, ooff)) in enumerate(zip(WRITER_SIZES, where)):
        s = R.apply(flat[moff:moff + H * W].reshape(H, W), None, 0, 0, 5, 4)[2]
        assert np.array_equal(done[2][k], s) and morph[k].tolist() == s[5:8].tolist()


# ------------------------------------------------------------------------------------------------ the command line, in child processes
S, BATCH = 32, 4
SIZES = {"a_wide.png": (100, 75), "b_thin.png": (40, 3), "c_tall.png": (33, 47), "d_photo.jpg": (57, 21), "e_square.png": (64, 64), "f_same.png": (32, 32)}   # (W, H)
FLAGS = ["--img_size", str(S), "--batch_size", str(BATCH), "--num_workers", "0"]
TRAIN = ["--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4", "--epochs", "1", "--no-viz"]
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))
OLD_HEADER = "name,width,height,foreground_pixels,foreground_fraction,ymin,xmin,ymax,xmax"
MORPH = ["--close_radius", "2", "--fill_holes", "-1", "--open_radius", "1", "--min_area", "20", "--lesions", "2"]


def child(cmd, cwd, timeout=300):
    r = subprocess.run([sys.executable, "-m"] + cmd, cwd=cwd, env=ENV, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """A working directory with six pictures and one trained checkpoint of the segmentation baseline."""
    d = tmp_path_factory.mktemp("predict_morph")
    (d / "pics").mkdir()
    rng = np.random.default_rng(0)
    for name, (W, H) in SIZES.items():
        Image.fromarray(rng.integers(0, 256, size=(H, W), dtype=np.uint8)).save(d / "pics" / name)
    child(["src.models.baselines.segmentation", "--exp", "pm"] + FLAGS + TRAIN, d)
    assert os.path.isfile(d / "runs" / "pm" / "LN-INT" / "train" / "best_model.pth")
    return d


def predict(work, out, extra=()):
    return child(["src.models.predict", "--entry", "baselines.segmentation", "--images", "pics", "--out", out, *extra, "--", "--exp", "pm"] + FLAGS, work)


def in_process(work):
    """-> (model, per batch (names, RaggedBatch on the device, the model's S x S input)) with the child's checkpoint, on the pictures decoded here."""
    import importlib
    from src.datasets import folder
    from src.datasets.image_dir import ImageDir, ImageDirCollate
    from src.models import predict as P, supervised
    from uia_hip import functional as UF
    module = importlib.import_module("src.models.baselines.segmentation")
    args = module.get_args(["--exp", "pm"] + FLAGS)
    UF.set_compute_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    model = P.load_model(module, args, str(work / "runs" / "pm" / "LN-INT" / "train" / "best_model.pth"))
    ds = ImageDir(str(work / "pics"), S)
    resize = folder.ResizeStage(S, with_mask=True)
    out = []
    with torch.no_grad():
        for at in range(0, len(ds), BATCH):
            buf, desc, _, (names, _) = ImageDirCollate(S)([ds[i] for i in range(at, min(at + BATCH, len(ds)))])
            batch = folder.RaggedBatch(buf.to(DEV), desc)
            images, second = resize(batch, None)
            images, _ = supervised.SEGMENTATION.to_input(images, second, args.in_channels)
            out.append((names, batch, images.clone()))
    return model, out


def run_in_process(work, tmp, ensemble):
    """The writer in this process with the command line's settings -> (names, sizes, stats, lesion rows, sums, morphology rows)."""
    from src.utils.viz import NativeMaskWriter
    model, batches = in_process(work)
    w = NativeMaskWriter(tmp, overlay=True, min_area=20, lesions=2, close_radius=2, open_radius=1, fill_holes=-1, prob=ensemble)
    with torch.no_grad():
        for names, batch, images in batches:
            if ensemble:
                one = model(images).detach().float()
                w.submit(torch.stack([one, one]).contiguous(), batch, names, flips=[0, 0])
            else:
                w.submit(model(images).detach(), batch, names)
    done = w.close()
    cat = lambda parts: [row for b in parts for row in b]     # noqa: E731
    return ([n for b in done for n in b[0]], [s for b in done for s in b[1]], cat([b[2] for b in done]), cat(w.lesion_lists()), cat(w.sums()),
            cat(w.morphology_stats()))


@pytest.mark.parametrize("ensemble", [False, True], ids=["plain", "ensemble"])
def test_predict_child_process_with_the_flags(work, tmp_path, ensemble):
    from src.models import predict as P
    out = "out_ens" if ensemble else "out_morph"
    ck = str(work / "runs" / "pm" / "LN-INT" / "train" / "best_model.pth")
    predict(work, out, MORPH + (["--ensemble", ck, "--prob"] if ensemble else []))
    names, sizes, stats, lists, sums, morph = run_in_process(work, tmp_path / "here", ensemble)
    assert names == sorted(SIZES)
    for sub in ["masks", "overlays"] + (["probs"] if ensemble else []):
        for name in names:
            stem = os.path.splitext(name)[0] + ".png"
            assert open(work / out / sub / stem, "rb").read() == open(tmp_path / "here" / sub / stem, "rb").read(), (sub, name)
    text = open(work / out / "predictions.csv").read()
    assert text == P.seg_csv(names, sizes, stats, sums if ensemble else None, filtered=True, morphology=morph)
    assert open(work / out / "lesions.csv").read() == P.lesions_csv(names, lists)
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == (OLD_HEADER + (",mean_foreground_probability,mean_spread" if ensemble else "") + ",pixels_added,pixels_removed").split(",")
    assert sum(int(r[-2]) + int(r[-1]) for r in rows[1:]) > 0, "the morphology changed nothing: the test shows nothing"
    raw = work / "out_raw" / "masks"
    if not raw.exists():
        predict(work, "out_raw")
    for name, row, m in zip(names, rows[1:], morph):
        launch_mask = np.asarray(Image.open(raw / (os.path.splitext(name)[0] + ".png"))) != 0
        after = np.asarray(Image.open(work / out / "masks" / (os.path.splitext(name)[0] + ".png"))) != 0
        assert int(m[2]) == int(launch_mask.sum()) and int(row[3]) == int(after.sum()), name
        if ensemble:                                # the denominator is the launch's own mask, neither the morphology's nor the filter's result
            q = np.asarray(Image.open(work / out / "probs" / (os.path.splitext(name)[0] + ".png"))).astype(np.int64)
            assert row[9] == (f"{int(q[launch_mask].sum()) / (255 * int(launch_mask.sum())):.6f}" if launch_mask.any() else ""), (name, row)


def test_predict_child_process_without_the_flags_is_what_it_was(work):
    """One checkpoint, uia_seg_predict_native, the old header: the files byte for byte."""
    from src.models import predict as P
    from src.utils.viz import NativeMaskWriter, encode_png
    from uia_hip import ops
    predict(work, "out_plain")
    out = work / "out_plain"
    assert sorted(os.listdir(out)) == ["masks", "overlays", "predictions.csv"]
    model, batches = in_process(work)
    all_names, all_sizes, all_stats = [], [], []
    with torch.no_grad():
        for batch_names, batch, images in batches:
            logits = model(images).detach().float()
            geo = batch.desc[:, :3].tolist()
            sizes = [(H, W) for _, H, W in geo]
            where, total = NativeMaskWriter.layout(sizes, overlay=True)
            desc = torch.tensor([[off, H, W, moff, ooff, 0, 0, 0] for (off, H, W), (moff, ooff) in zip(geo, where)], dtype=torch.int32)
            flat = torch.zeros(total, dtype=torch.uint8, device=DEV)
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
