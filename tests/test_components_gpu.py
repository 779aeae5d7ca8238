"""-m gpu: uia_mask_components (csrc/components.hip) against the host flood fill of tests/components_reference.py, by exact equality of mask bytes, overlay
bytes, stats and list, with sentinel bytes and words round every range; then the same through src/utils/viz.NativeMaskWriter and through a child process
of src/models/predict.py.  The kernel's tile is 32 rows x 64 columns: 33 x 65 is a tile plus one both ways, 130 x 70 and 70 x 130 are several tiles plus a
remainder down and across."""
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

import components_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BYTE, SENT_WORD = 0xA5, -0x5A5A5A5B
SMALL = [(1, 1), (1, 37), (37, 1), (7, 5), (33, 65), (130, 70), (70, 130)]
PARAMS = [(min_area, keep, conn) for min_area in (0, 1, 2, 50) for keep in (0, 1, 3) for conn in (4, 8)]
MAX_LISTS = (0, 1, 5, 32)
_LABELLED = {}


def labelled(H, W, name):
    """The pattern `name` at H x W, labelled once for the whole module and never changed."""
    if (H, W) not in _LABELLED:
        _LABELLED[(H, W)] = {k: R.Labelled(m) for k, m in R.patterns(H, W).items()}
    return _LABELLED[(H, W)][name]


def overlay_of(mask, seed):
    g = np.random.default_rng(seed).integers(0, 256, size=mask.shape, dtype=np.uint8)
    return np.stack([g, np.maximum(g, mask), g], axis=-1)


def lay_out(images, start):
    """images: [(Labelled, overlay or None, min_area, keep, conn)] -> (host buffer with sentinel bytes before, between and after the ranges, desc int32
    [B, 8], [(mask offset, overlay offset)]).  Gaps of 1 .. 3 bytes keep the offsets of every alignment."""
    at, where, parts = start, [], [np.full(start, SENT_BYTE, np.uint8)]
    for k, (lab, over, _, _, _) in enumerate(images):
        moff, at = at, at + lab.mask.size
        parts.append(lab.mask.ravel())
        gap = 1 + k % 3
        parts.append(np.full(gap, SENT_BYTE, np.uint8))
        at += gap
        ooff = -1
        if over is not None:
            ooff, at = at, at + over.size
            parts += [over.ravel(), np.full(gap, SENT_BYTE, np.uint8)]
            at += gap
        where.append((moff, ooff))
    desc = np.array([[moff, *lab.mask.shape, ooff, min_area, keep, conn, 0] for (lab, _, min_area, keep, conn), (moff, ooff) in zip(images, where)], dtype=np.int32)
    return np.concatenate(parts), desc, where


def launch(buf, desc, max_list):
    """One call of the C entry on the device buffer `buf` with stats and list inside larger tensors of sentinel words -> (stats, list) on the host."""
    from uia_hip import _lib, ops
    B = desc.shape[0]
    stats = torch.full((8 + B * 8 + 8,), SENT_WORD, dtype=torch.int32, device=DEV)
    rows = torch.full((8 + B * max_list * 8 + 8,), SENT_WORD, dtype=torch.int32, device=DEV)
    ws = ops.mask_components_workspace(B, int((desc[:, 1].astype(np.int64) * desc[:, 2]).sum()), torch.device(DEV))
    hdesc = torch.from_numpy(np.ascontiguousarray(desc))
    rc = _lib.lib().uia_mask_components(torch.cuda.current_stream().cuda_stream, B, buf.data_ptr(), buf.numel(), hdesc.data_ptr(), ws.data_ptr(), ws.numel(),
                                        stats[8:].data_ptr(), rows[8:].data_ptr() if max_list else None, max_list)
    assert rc == 0, _lib.lib().uia_last_error().decode()
    torch.cuda.synchronize()
    stats, rows = stats.cpu().numpy(), rows.cpu().numpy()
    for t in (stats, rows):
        assert (t[:8] == SENT_WORD).all() and (t[-8:] == SENT_WORD).all(), "a word beside stats or list was written"
    return stats[8:-8].reshape(B, 8), rows[8:-8].reshape(B, max_list, 8)


def expected(images, where, host, max_list):
    """The buffer, stats and list the contract asks for."""
    want = host.copy()
    stats, rows = [], []
    for (lab, over, min_area, keep, conn), (moff, ooff) in zip(images, where):
        m, o, s, r = lab.apply(over, min_area, keep, conn, max_list)
        want[moff:moff + m.size] = m.ravel()
        if o is not None:
            want[ooff:ooff + o.size] = o.ravel()
        stats.append(s)
        rows.append(r)
    return want, np.stack(stats), np.stack(rows)


def describe(images, k):
    lab, over, min_area, keep, conn = images[k]
    return f"image {k}: {lab.mask.shape}, overlay={over is not None}, min_area={min_area}, keep={keep}, connectivity={conn}"


def run_and_compare(images, max_list, start=1):
    host, desc, where = lay_out(images, start)
    buf = torch.from_numpy(host).to(DEV)
    stats, rows = launch(buf, desc, max_list)
    got = buf.cpu().numpy()
    want, wstats, wrows = expected(images, where, host, max_list)
    for k in range(len(images)):
        assert np.array_equal(stats[k], wstats[k]), (describe(images, k), stats[k], wstats[k])
        assert np.array_equal(rows[k], wrows[k]), (describe(images, k), max_list, rows[k], wrows[k])
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"byte {at} of the buffer is {got[at]}, expected {want[at]} (was {host[at]}); ranges {where}")
    return buf, desc, stats, rows, host


def grid_images(H, W, names, params):
    out = []
    for name in names:
        for k, (min_area, keep, conn) in enumerate(params):
            lab = labelled(H, W, name)
            out.append((lab, overlay_of(lab.mask, len(out)) if (len(out) + k) % 2 == 0 else None, min_area, keep, conn))
    return out


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("max_list", MAX_LISTS)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_content_and_parameter(shape, max_list):
    """Every content x min_area x keep x connectivity at one shape in one call: one image per combination, every second one with an overlay."""
    run_and_compare(grid_images(*shape, sorted(R.patterns(*shape)), PARAMS), max_list, start=1 + max_list % 4)


@pytest.mark.parametrize("max_list", MAX_LISTS)
def test_several_tiles_both_ways(max_list):
    """300 x 517: ten tiles down, nine across, a remainder both ways; the contents whose components cross the most seams."""
    params = [(0, 0, 8), (0, 0, 4), (2, 1, 4), (1, 3, 8), (50, 3, 4), (50, 0, 8), (2, 3, 4), (0, 1, 8)]
    run_and_compare(grid_images(300, 517, ["spiral", "checkerboard", "random0.5", "random0.6", "corner", "values", "rings", "full"], params), max_list, start=3)


def test_checkerboard_keep_three_keeps_the_first_three_pixels():
    lab = labelled(33, 65, "checkerboard")
    _, _, stats, rows, _ = run_and_compare([(lab, None, 0, 3, 4), (lab, None, 0, 3, 8)], 5)
    assert stats[0].tolist() == [3, 0, 0, 0, 4, 1073, 3, 1073] and rows[0, :, 5].tolist() == [0, 2, 4, 0, 0]
    assert stats[1, 5:].tolist() == [1, 1, 1073] and rows[1, 0, 0] == 1073


def test_a_keep_beyond_the_list_limit():
    """keep is not bounded by the 32 rows of the list: the 40 and the 200 largest of 1073 one-pixel components, and of a random mask's."""
    images = [(labelled(33, 65, "checkerboard"), None, 0, 40, 4), (labelled(130, 70, "random0.3"), overlay_of(labelled(130, 70, "random0.3").mask, 1), 0, 200, 4),
              (labelled(130, 70, "random0.3"), None, 2, 40, 8), (labelled(7, 5, "corner"), None, 0, 1000, 4)]
    for max_list in (0, 32):
        run_and_compare(images, max_list)


def test_coordinate_sums_beyond_32_bits():
    """16384 x 64, the tallest image the entry takes, cut into three pieces: 512 tiles down, and a sum of y of 4.9e9 that only 64-bit sums hold."""
    m = np.full((16384, 64), 255, np.uint8)
    m[5000, :] = 0
    m[5001:, 40] = 0
    lab = R.Labelled(m)
    assert int(lab.parts(4)[2]["sy"].max()) > 2 ** 32
    _, _, stats, rows, _ = run_and_compare([(lab, None, 0, 0, 4), (lab, None, 300000, 2, 8)], 3)
    assert rows[0, :, 6].tolist() == [10692, 2499, 10692] and stats[1, 5:].tolist() == [3, 2, 1037129]


def test_ragged_batch_with_different_parameters():
    """Five images of different sizes in one buffer from an odd offset, overlays on some, parameters that differ."""
    images = [(labelled(1, 1, "full"), None, 0, 0, 8), (labelled(7, 5, "checkerboard"), overlay_of(labelled(7, 5, "checkerboard").mask, 2), 0, 3, 4),
              (labelled(33, 65, "spiral"), overlay_of(labelled(33, 65, "spiral").mask, 3), 50, 1, 4), (labelled(130, 70, "random0.5"), None, 2, 3, 8),
              (labelled(37, 1, "values"), overlay_of(labelled(37, 1, "values").mask, 4), 1, 0, 4)]
    for max_list in (0, 5):
        run_and_compare(images, max_list, start=7)


def test_two_calls_agree_and_a_second_pass_changes_nothing():
    images = grid_images(130, 70, ["random0.3", "random0.6", "values", "rings", "corner"], [(2, 3, 4), (50, 1, 8), (0, 0, 8), (1, 3, 8)])
    first = run_and_compare(images, 5)
    again = run_and_compare(images, 5)
    assert torch.equal(first[0], again[0]) and np.array_equal(first[2], again[2]) and np.array_equal(first[3], again[3])
    buf, desc, stats, rows, _ = first
    before = buf.clone()
    stats2, rows2 = launch(buf, desc, 5)                          # the first call's output, the same parameters
    assert torch.equal(buf, before) and np.array_equal(rows2, rows)
    assert np.array_equal(stats2[:, :5], stats[:, :5]) and np.array_equal(stats2[:, 5], stats2[:, 6]) and np.array_equal(stats2[:, 6], stats[:, 6])
    assert np.array_equal(stats2[:, 7], stats[:, 0])


def test_the_wrapper_returns_what_the_entry_writes():
    from uia_hip import ops
    images = grid_images(33, 65, ["random0.5", "corner"], [(2, 3, 4), (0, 1, 8)])
    host, desc, where = lay_out(images, 1)
    buf = torch.from_numpy(host).to(DEV)
    stats, rows = ops.mask_components(buf, torch.from_numpy(desc), max_list=5)
    assert stats.is_cuda and rows.is_cuda and tuple(stats.shape) == (4, 8) and tuple(rows.shape) == (4, 5, 8)
    want, wstats, wrows = expected(images, where, host, 5)
    assert np.array_equal(buf.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), wstats) and np.array_equal(rows.cpu().numpy(), wrows)
    stats, rows = ops.mask_components(buf, torch.from_numpy(desc))
    assert tuple(rows.shape) == (4, 0, 8) and np.array_equal(stats.cpu().numpy()[:, :5], wstats[:, :5])


# ------------------------------------------------------------------------------------------------ NativeMaskWriter
WRITER_S = 32
WRITER_SIZES = [(75, 100), (47, 33), (64, 64), (21, 57)]          # (H, W)


def synthetic_batch():
    """Four gray pictures of different sizes as a folder.RaggedBatch on the device, and logits whose arg-max has blobs and speckle."""
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


def test_writer_defaults_enqueue_nothing_new_and_filtering_matches_the_reference(tmp_path, monkeypatch):
    from src.utils import viz
    from uia_hip import ops
    batch, logits, pics, names = synthetic_batch()

    def write(out, **kw):
        w = viz.NativeMaskWriter(tmp_path / out, overlay=True, **kw)
        w.submit(logits, batch, names)
        done = w.close()
        return done, w.lesion_lists()

    real = ops.mask_components
    monkeypatch.setattr(ops, "mask_components", lambda *a, **k: (_ for _ in ()).throw(AssertionError("mask_components was called with the defaults")))
    (plain,), none = write("plain")
    (explicit,), none2 = write("explicit", min_area=0, keep=0, connectivity=8, lesions=0)
    monkeypatch.setattr(ops, "mask_components", real)
    assert none == [] and none2 == [] and files_of(tmp_path / "plain") == files_of(tmp_path / "explicit")
    assert plain[0] == explicit[0] == names and plain[1] == explicit[1] == WRITER_SIZES and np.array_equal(plain[2], explicit[2])

    # the unfiltered masks and overlays, from the same launch the writer makes
    where, total = viz.NativeMaskWriter.layout(WRITER_SIZES, True)
    desc = torch.tensor([[off, H, W, moff, ooff, 0, 0, 0] for (off, H, W), (moff, ooff) in zip(batch.desc[:, :3].tolist(), where)], dtype=torch.int32)
    flat = torch.zeros(total, dtype=torch.uint8, device=DEV)
    ops.seg_predict_native(logits, batch.data, desc, flat)
    flat = flat.cpu().numpy()
    (done,), (lists,) = write("largest", keep=1, lesions=4)
    assert done[0] == names and lists.shape == (4, 4, 8) and lists.dtype == np.int32
    more_than_one = 0
    for k, ((H, W), (moff, ooff)) in enumerate(zip(WRITER_SIZES, where)):
        mask, over = flat[moff:moff + H * W].reshape(H, W), flat[ooff:ooff + 3 * H * W].reshape(H, W, 3)
        assert np.array_equal(over, np.stack([pics[k], np.maximum(pics[k], mask), pics[k]], axis=-1))
        m, o, stats, rows = R.apply(mask, over, keep=1, connectivity=8, max_list=4)
        more_than_one += stats[5] > 1
        viz.write_png(tmp_path / "want_mask.png", m, viz.PNG_LEVEL)
        viz.write_png(tmp_path / "want_over.png", o, viz.PNG_LEVEL)
        stem = names[k][:-4]
        assert open(tmp_path / "largest" / "masks" / f"{stem}.png", "rb").read() == open(tmp_path / "want_mask.png", "rb").read(), names[k]
        assert open(tmp_path / "largest" / "overlays" / f"{stem}.png", "rb").read() == open(tmp_path / "want_over.png", "rb").read(), names[k]
        assert np.array_equal(done[2][k], stats) and np.array_equal(lists[k], rows), (names[k], done[2][k], stats)
        assert np.array_equal(plain[2][k][:5], R.apply(mask)[2][:5])
    assert more_than_one >= 2, "the synthetic logits must give the filter something to remove"


# ------------------------------------------------------------------------------------------------ the command line, in a child process
def test_predict_child_process_with_and_without_the_flags(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from src.models import predict as P
    S, sizes = 32, {"a_wide.png": (100, 75), "b_thin.png": (40, 3), "c_tall.png": (33, 47), "d_photo.jpg": (57, 21), "e_square.png": (64, 64), "f_same.png": (32, 32)}
    flags = ["--img_size", str(S), "--batch_size", "4", "--num_workers", "0"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "nextgen-uia_amd"), ROOT]))
    (tmp_path / "pics").mkdir()
    rng = np.random.default_rng(0)
    for name, (W, H) in sizes.items():
        Image.fromarray(rng.integers(0, 256, size=(H, W), dtype=np.uint8)).save(tmp_path / "pics" / name)

    def child(cmd):
        r = subprocess.run([sys.executable, "-m"] + cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    child(["src.models.baselines.segmentation", "--exp", "pc"] + flags + ["--synthetic", "--synthetic_train", "8", "--synthetic_val", "4", "--synthetic_test", "4",
                                                                         "--epochs", "1", "--no-viz"])
    base = ["src.models.predict", "--entry", "baselines.segmentation", "--images", "pics"]
    child(base + ["--out", "raw", "--", "--exp", "pc"] + flags)
    child(base + ["--out", "one", "--keep_largest", "1", "--lesions", "4", "--", "--exp", "pc"] + flags)
    assert sorted(os.listdir(tmp_path / "raw")) == ["masks", "overlays", "predictions.csv"]
    assert sorted(os.listdir(tmp_path / "one")) == ["lesions.csv", "masks", "overlays", "predictions.csv"]
    names = sorted(sizes)
    stats, lists = [], []
    for name in names:
        stem = os.path.splitext(name)[0]
        mask, over = (np.asarray(Image.open(tmp_path / "raw" / sub / f"{stem}.png")) for sub in ("masks", "overlays"))
        m, o, s, rows = R.apply(mask, over, keep=1, connectivity=8, max_list=4)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "one" / "masks" / f"{stem}.png")), m), name
        assert np.array_equal(np.asarray(Image.open(tmp_path / "one" / "overlays" / f"{stem}.png")), o), name
        stats.append(s)
        lists.append(rows)
    hw = [(sizes[n][1], sizes[n][0]) for n in names]
    assert open(tmp_path / "one" / "predictions.csv").read() == P.seg_csv(names, hw, stats)
    assert open(tmp_path / "one" / "lesions.csv").read() == P.lesions_csv(names, lists)
    assert open(tmp_path / "raw" / "predictions.csv").read() == P.seg_csv(names, hw, [R.apply(np.asarray(Image.open(tmp_path / "raw" / "masks" / f"{os.path.splitext(n)[0]}.png")))[2]
                                                                                     for n in names])
