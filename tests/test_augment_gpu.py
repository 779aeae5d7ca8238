"""-m gpu: uia_augment_batch (csrc/augment.hip) against the numpy restatement of tests/augment_reference.py — which tests/test_augment_host.py holds to PIL
itself — pixel for pixel; the blur against its float64 value; empty programs bit for bit; masks following the geometry; S = 518; operands one element
into their buffers; refusals that leave the outputs alone; and the three training loops with the stage on, off and on the synthetic noise."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import augment_reference as R  # noqa: E402
from guarded_out import dev  # noqa: E402

SIZES = (37, 64)
GUARD = 64


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "augment_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def batch(S):
    """B = 3: the fixtures' three 8-bit planes as k / 255, one of them perturbed off the 8-bit grid (the kernel quantises once), and their masks."""
    z = golden()
    x = (z[f"in_{S}"].astype(np.float32) / np.float32(255))[:, None].copy()
    rng = np.random.default_rng(S)
    x[2, 0] = np.clip(x[2, 0] + rng.uniform(-0.45, 0.45, (S, S)).astype(np.float32) / np.float32(255), 0, 1)
    return x, z[f"mask_{S}"][:, None].copy()


class Guarded:
    """A device tensor at `offset` elements inside a sentinel-filled buffer."""

    def __init__(self, shape, dtype, offset=GUARD, fill=None):
        self.n, self.offset = math.prod(shape), offset
        self.sentinel = fill if fill is not None else (float("nan") if dtype == torch.float32 else 0xA5)
        self.buf = torch.full((offset + self.n + GUARD,), self.sentinel, dtype=dtype, device=dev())
        self.t = self.buf[offset:offset + self.n].view(shape)

    def untouched(self, whole=False):
        b = self.buf.cpu()
        parts = [b] if whole else [b[:self.offset], b[self.offset + self.n:]]
        return all(bool(torch.isnan(p).all()) if isinstance(self.sentinel, float) and math.isnan(self.sentinel) else bool((p == self.sentinel).all()) for p in parts)


def run(x, m, table, offset=GUARD, in_offset=0):
    """The kernel on numpy inputs -> numpy outputs; outputs sit in guarded buffers (offset: elements into them), inputs `in_offset` elements into theirs."""
    from uia_hip import ops
    xi = Guarded(x.shape, torch.float32, offset=in_offset, fill=0.0)
    xi.t.copy_(torch.from_numpy(x))
    oi = Guarded(x.shape, torch.float32, offset=offset)
    mi = om = None
    if m is not None:
        mi = Guarded(m.shape, torch.uint8, offset=in_offset, fill=0)
        mi.t.copy_(torch.from_numpy(m))
        om = Guarded(m.shape, torch.uint8, offset=offset)
    ops.augment_batch(xi.t, None if mi is None else mi.t, torch.from_numpy(np.ascontiguousarray(table)), oi.t, None if om is None else om.t)
    torch.cuda.synchronize()
    assert oi.untouched() and (om is None or om.untouched()), "a write outside the outputs"
    return oi.t.cpu().numpy(), None if om is None else om.t.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def check_equal(x, m, table, **kw):
    got_i, got_m = run(x, m, table, **kw)
    want_i, want_m = R.augment_batch(x, m, table)
    for b in range(x.shape[0]):
        d = np.abs(np.rint(got_i[b] * 255) - np.rint(want_i[b] * 255))
        assert same_bits(got_i[b], want_i[b]), f"image {b} (program {table[b, 1:1 + table[b, 0, 0]].tolist()}): {(d > 0).sum()} pixels differ, max {d.max():.0f} grey levels"
        if m is not None:
            assert np.array_equal(got_m[b], want_m[b]), f"mask {b}: {(got_m[b] != want_m[b]).sum()} pixels differ"


ALONE = {
    "identity": [[(R.IDENTITY, 0, 0, 0)], [(R.IDENTITY, 0, 0, 0), (R.IDENTITY, 0, 0, 0)]],
    "autocontrast": [[(R.AUTOCONTRAST, 0, 0, 0)]] * 2,
    "equalize": [[(R.EQUALIZE, 0, 0, 0)]] * 2,
    "contrast": [[(R.CONTRAST, 0.7500001, 0, 0)], [(R.CONTRAST, 1.25, 0, 0)]],
    "brightness": [[(R.BRIGHTNESS, 0.8123, 0, 0)], [(R.BRIGHTNESS, 1.25, 0, 0)]],
    "sharpness": [[(R.SHARPNESS, 0.76, 0, 0)], [(R.SHARPNESS, 1.2345, 0, 0)]],
    "posterize": [[(R.POSTERIZE, 4, 0, 0)], [(R.POSTERIZE, 7, 0, 0)]],
    "solarize": [[(R.SOLARIZE, 1, 0, 0)], [(R.SOLARIZE, 201, 0, 0)]],
    "hflip": [[(R.HFLIP, 0, 0, 0)]] * 2,
    "vflip": [[(R.VFLIP, 0, 0, 0)]] * 2,
}


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("op", sorted(ALONE) + ["crop"])
def test_each_op_alone_equals_the_restatement(op, S):
    """Images 0 and 2 run one op (two parameter choices), image 1 has an empty program and must come back bit for bit."""
    x, m = batch(S)
    lo = int(np.ceil(np.sqrt(0.8) * S))
    a, b = ALONE[op] if op != "crop" else ([(R.CROP, S - lo, S - lo, lo)], [(R.CROP, 1, 0, S - 1)])
    table = R.make_table([a, [], b], with_mask=True)
    check_equal(x, m, table)
    got_i, got_m = run(x, m, table)
    assert same_bits(got_i[1], x[1]) and np.array_equal(got_m[1], m[1])


@pytest.mark.parametrize("S", SIZES)
def test_thirteen_op_program_with_repeats_and_two_crops_equals_the_restatement(S):
    """The fixtures' composed programs (the 13-op one is the longest the sampler can draw), here on all three images at once and without masks as well."""
    z = golden()
    names = [str(n) for n in z[f"name_{S}"]]
    table = np.stack([z[f"tab_{S}"][names.index(n)] for n in ("composed13", "composed_weak", "composed_strong")])
    assert table[0, 0, 0] == 13 and (table[0, 1:, 0] == R.CROP).sum() == 2
    x, m = batch(S)
    check_equal(x, m, table)
    table[:, 0, 1] = 0
    check_equal(x, None, table)


@pytest.mark.parametrize("S", SIZES)
def test_blur_is_within_one_level_and_equal_away_from_rounding_ties(S):
    """The kernel's fp32 sums against the float64 Gaussian: never more than one grey level off, and equal wherever the float64 value lies more than 1e-3 from
    a rounding tie (an 11-tap convex fp32 sum of 8-bit values errs by less than 2e-4); fewer than 1 % of the pixels are inside that band."""
    x, m = batch(S)
    for sigmas in ((0.75, 1.0, 1.25), (1.1337, 0.9, 0.8)):
        table = R.make_table([[(R.BLUR, s, 0, 0)] for s in sigmas], with_mask=True)
        got_i, got_m = run(x, m, table)
        assert np.array_equal(got_m, m)
        for b, s in enumerate(sigmas):
            u = R.quantise(x[b, 0])
            exact = R.gaussian_blur_exact(u, s) + 0.5
            want = np.clip(np.floor(exact), 0, 255)
            got = np.rint(got_i[b, 0] * np.float32(255))
            assert same_bits(got_i[b, 0], R.dequantise(got.astype(np.uint8)))                  # the output is some 8-bit level / 255
            d = np.abs(got - want)
            away = np.abs(exact - np.round(exact)) > 1e-3
            assert away.mean() > 0.99
            print(f"S={S} sigma={s}: max |kernel - float64| = {d.max():.0f} levels, {int((d > 0).sum())} pixels differ, {int((~away).sum())} within 1e-3 of a tie")
            assert d.max() <= 1 and not (d[away] > 0).any()


def test_empty_programs_return_the_input_bits():
    """Floats off the 8-bit grid, outside [0, 1], NaN and -0.0 among them, and arbitrary mask bytes: nothing is round-tripped through 8 bits."""
    rng = np.random.default_rng(7)
    S = 37
    x = rng.uniform(-0.5, 1.5, (3, 1, S, S)).astype(np.float32)
    x[0, 0, 0, :5] = [np.nan, -0.0, np.inf, 1e-40, 1.0]
    m = rng.integers(0, 256, (3, 1, S, S)).astype(np.uint8)
    table = R.make_table([[], [], []], with_mask=True)
    for kw in (dict(), dict(offset=GUARD + 1, in_offset=1)):
        got_i, got_m = run(x, m, table, **kw)
        assert same_bits(got_i, x) and np.array_equal(got_m, m)
    got_i, _ = run(x, None, R.make_table([[], [], []]))
    assert same_bits(got_i, x)


@pytest.mark.parametrize("S", SIZES)
def test_mask_follows_the_geometry_of_the_image(S):
    """A crop with odd offsets and both flips, on a mask of arbitrary bytes: the mask is moved, never interpreted — and it is the image's own geometry (an
    image that IS its mask's bytes stays equal to it under flips)."""
    rng = np.random.default_rng(S)
    m = rng.integers(0, 256, (3, 1, S, S)).astype(np.uint8)
    m[2] = (rng.random((1, S, S)) < 0.5) * 255
    x = m.astype(np.float32) / np.float32(255)
    table = R.make_table([[(R.CROP, 1, 3, S - 4), (R.HFLIP, 0, 0, 0), (R.VFLIP, 0, 0, 0)], [(R.VFLIP, 0, 0, 0), (R.HFLIP, 0, 0, 0), (R.VFLIP, 0, 0, 0)],
                          [(R.HFLIP, 0, 0, 0), (R.CROP, 3, 1, S - 3), (R.CROP, 0, 0, S), (R.IDENTITY, 0, 0, 0)]], with_mask=True)
    check_equal(x, m, table)
    got_i, got_m = run(x, m, table)
    assert np.array_equal(np.rint(got_i[1] * 255).astype(np.uint8), got_m[1]) and np.array_equal(got_m[1, 0], m[1, 0, :, ::-1])
    want_m0 = R.crop_resize_nearest(m[0, 0], 1, 3, S - 4)[::-1, ::-1]
    assert np.array_equal(got_m[0, 0], want_m0)


def test_one_image_of_518_pixels_a_side():
    """DINOv2's size: the planes do not fit LDS, a thread owns 262 pixels, the resample tables have 518 entries; side = 464 is one of the crops at which PIL's
    stepped nearest coordinate lands below an integer (d = 129, 388)."""
    S = 518
    rng = np.random.default_rng(518)
    yy, xx = np.mgrid[0:S, 0:S]
    u = np.clip(rng.gamma(2.0, 0.2, (S, S)) * (0.5 + 0.5 * np.sin(yy / 17.0) * np.cos(xx / 23.0)) * 255 * (np.hypot(yy - 100, xx - 259) < 380), 0, 255).astype(np.uint8)
    x = (u.astype(np.float32) / np.float32(255))[None, None]
    m = (np.hypot(yy - 260, xx - 240) < 120).astype(np.uint8)[None, None]
    assert [int(v) for v in R.nearest_index(464, S)[[129, 388]]] == [115, 347]
    table = R.make_table([[(R.CONTRAST, 1.2, 0, 0), (R.EQUALIZE, 0, 0, 0), (R.SHARPNESS, 0.8, 0, 0), (R.CROP, 31, 17, 464), (R.HFLIP, 0, 0, 0), (R.AUTOCONTRAST, 0, 0, 0),
                           (R.VFLIP, 0, 0, 0), (R.SOLARIZE, 200, 0, 0), (R.POSTERIZE, 5, 0, 0), (R.BRIGHTNESS, 1.1, 0, 0)]], with_mask=True)
    check_equal(x, m, table)


@pytest.mark.parametrize("S", SIZES)
def test_operands_one_element_into_their_buffers(S):
    """Images and outputs 4 bytes, masks 1 byte off a 16-byte boundary: the scalar path of the fp32 loads and stores gives the same pixels."""
    z = golden()
    names = [str(n) for n in z[f"name_{S}"]]
    table = np.stack([z[f"tab_{S}"][names.index("composed13")], R.make_table([[]], with_mask=True)[0], z[f"tab_{S}"][names.index("composed_weak")]])
    x, m = batch(S)
    for off_out, off_in in ((GUARD + 1, 1), (GUARD + 1, 0), (GUARD, 3)):
        check_equal(x, m, table, offset=off_out, in_offset=off_in)


def test_refusals_return_non_zero_and_leave_the_outputs_untouched():
    from uia_hip import _lib, ops
    lib = _lib.lib()
    S, B = 37, 3
    x, m = batch(S)
    xi, mi = torch.from_numpy(x).to(dev()), torch.from_numpy(m).to(dev())
    oi, om = Guarded(x.shape, torch.float32), Guarded(m.shape, torch.uint8)
    ws = ops.augment_workspace(B, S, dev())
    good = R.make_table([[(R.HFLIP, 0, 0, 0)], [], [(R.EQUALIZE, 0, 0, 0)]], with_mask=True)
    st = torch.cuda.current_stream().cuda_stream

    def call(tab=good, B=B, images=xi.data_ptr(), masks=mi.data_ptr(), wsp=ws.data_ptr(), out_images=oi.t.data_ptr(), out_masks=om.t.data_ptr()):
        tab = None if tab is None else np.ascontiguousarray(tab, dtype=np.int32)
        return lib.uia_augment_batch(st, B, S, images, masks, None if tab is None else tab.ctypes.data, wsp, ws.numel(), out_images, out_masks)

    def tab_with(row, n=1, image=2):
        t = good.copy()
        t[image, 0, 0], t[image, 1] = n, row
        return t

    for what, kw in [("unknown opcode", dict(tab=tab_with((12, 0, 0, 0)))), ("crop leaving the image", dict(tab=tab_with((R.CROP, 4, 0, 34)))),
                     ("crop larger than the image", dict(tab=tab_with((R.CROP, 0, 0, 38)))), ("more than 13 ops", dict(tab=tab_with((R.IDENTITY, 0, 0, 0), n=14))),
                     ("null images", dict(images=None)), ("null outputs", dict(out_images=None)), ("null table", dict(tab=None)), ("null workspace", dict(wsp=None)),
                     ("masks without an output", dict(out_masks=None)), ("B = 0", dict(B=0))]:
        assert call(**kw) != 0, what
        assert lib.uia_last_error()
    torch.cuda.synchronize()
    assert oi.untouched(whole=True) and om.untouched(whole=True)
    assert call() == 0                                              # and the same buffers take a good table
    torch.cuda.synchronize()
    want_i, want_m = R.augment_batch(x, m, good)
    assert same_bits(oi.t.cpu().numpy(), want_i) and np.array_equal(om.t.cpu().numpy(), want_m)
    with pytest.raises(_lib.UiaError):
        ops.augment_batch(torch.from_numpy(x), None, torch.from_numpy(R.make_table([[], [], []])))      # CPU tensors
    from src.datasets import augment as A
    with pytest.raises(ValueError):
        A.BatchAugmenter(True, True, True, seed=1)(xi)                                                  # a stage made for masks, and no mask
    with pytest.raises(ValueError):
        A.BatchAugmenter(True, True, False, seed=1)(xi[:, :, :, :36].contiguous())                      # not square
    assert call(out_images=xi.data_ptr() + 4 * S * S) != 0 and call(out_masks=mi.data_ptr() + 8) != 0   # outputs overlapping the inputs


def test_stage_draws_launches_and_counts_without_touching_global_generators():
    """BatchAugmenter on a device batch: what it returns is what the kernel makes of the table it drew (bit for bit the direct call's result), which is the
    restatement's for every program without a blur; the count is the number of non-empty programs, and the batch of the next call gets another table.
    A blur may round a pixel within 1e-3 of a tie the other way, and the ops behind it (a histogram table, a solarize) can turn that one level into many, so
    a blurred image is held to the restatement — within one grey level — only where nothing but crops, flips and identities follow its single blur: a crop's
    two convex fixed-point passes keep a difference of at most one level at most one level."""
    from src.datasets import augment as A
    from uia_hip import ops
    S = 64
    x, m = batch(S)
    xi, mi = torch.from_numpy(x).to(dev()), torch.from_numpy(m).to(dev())
    torch.manual_seed(5)
    before = torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()
    st = A.BatchAugmenter(True, True, True, seed=9, rank=1)
    st.set_epoch(2)
    tables, n, blurred = [], 0, 0
    for it in range(A.BatchAugmenter.DEPTH + 2):                   # past the ring of pinned tables
        oi, om = st(xi, mi)
        t = A.draw_programs(3, S, True, True, True, A.make_rng(9, 1, 2, it))
        want_i, want_m = R.augment_batch(x, m, t)
        got_i = oi.cpu().numpy()
        di, dm = ops.augment_batch(xi, mi, torch.from_numpy(t))
        assert same_bits(got_i, di.cpu().numpy()) and torch.equal(om, dm), it
        for b in range(3):
            codes = t[b, 1:1 + t[b, 0, 0], 0].tolist()
            if R.BLUR not in codes:
                assert same_bits(got_i[b], want_i[b]), (it, b)
            elif codes.count(R.BLUR) == 1 and all(c in (R.IDENTITY, R.CROP, R.HFLIP, R.VFLIP) for c in codes[codes.index(R.BLUR) + 1:]):
                assert np.abs(np.rint(got_i[b] * 255) - np.rint(want_i[b] * 255)).max() <= 1, (it, b)
                blurred += 1
            assert np.array_equal(om[b].cpu().numpy(), want_m[b])
        n += int((t[:, 0, 0] > 0).sum())
        tables.append(t)
    assert st.augmented == n > 0 and blurred >= 2 and any(not np.array_equal(tables[0], t) for t in tables[1:])
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state())


# ------------------------------------------------------------------------------------------------ the training loops
def _seg_blob(path, S=32, n=24):
    g = torch.Generator().manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    cx = torch.randint(S // 4, 3 * S // 4, (n,), generator=g)
    labels = (((yy[None] - S // 2) ** 2 + (xx[None] - cx[:, None, None]) ** 2) <= (S // 5) ** 2)[:, None].to(torch.uint8) * 255
    images = (torch.randint(0, 120, (n, 1, S, S), generator=g) + labels // 2).to(torch.uint8)
    torch.save({"images": images, "labels": labels, "split": {"train": list(range(16)), "val": list(range(16, 20)), "test": list(range(20, 24))}}, path)
    return images, labels


LOOP = ["--batch_size", "4", "--epochs", "6", "--val_every", "5", "--num_workers", "0", "--lr", "1e-3"]      # 24 iterations, one validation at the end
SYNTHETIC = ["--synthetic", "--synthetic_train", "16", "--synthetic_val", "4", "--synthetic_test", "4"]


def _three_runs(train, base, data, tmp_path):
    """The loop with the default flags on the data file, with both flags off, and on the synthetic noise.  Each run must train to a finite loss: the
    training losses the loop logs (iterations 0, 10 and 20 of 24: before any update and after ten and twenty of them) and the validation loss after
    the last epoch, read back from <train dir>/log/scalars.jsonl."""
    import json
    outs = []
    for k, extra in enumerate((["--data_pt", data], ["--data_pt", data, "--no-strong_augs", "--no-weak_augs"], SYNTHETIC)):
        where = tmp_path / f"train{k}"
        os.makedirs(where, exist_ok=True)
        out = train(base + LOOP + extra, str(where))
        rows = [json.loads(line) for line in open(where / "log" / "scalars.jsonl")]
        tr = [r["value"] for r in rows if r["tag"].endswith("/train_loss")]
        va = [r["value"] for r in rows if r["tag"].endswith("/val_loss")]
        assert out["iters"] == 24 and len(tr) == 3 and len(va) == 1, (k, out["iters"], tr, va)
        assert all(math.isfinite(v) for v in tr + va), (k, tr, va)
        outs.append(out)
    on, off, syn = outs
    assert on["augmented_images"] > 0, on
    assert off["augmented_images"] == 0 and syn["augmented_images"] == 0
    return outs


def test_segmentation_loop_applies_the_stage_to_data_pt_batches_only(tmp_path, monkeypatch):
    from src.models.baselines import segmentation as S
    from src.models.biomedclip import segmentation as L
    monkeypatch.chdir(tmp_path)
    _seg_blob(tmp_path / "seg.pt", S=64)

    def train(argv, where):
        args = S.get_args(argv)
        args.train_snapshot_path = where
        torch.manual_seed(args.seed)
        return L.train(args, S.prepare_model)

    for out in _three_runs(train, ["--img_size", "64", "--dtype", "fp32"], str(tmp_path / "seg.pt"), tmp_path):
        assert math.isfinite(out["last_loss"])


def test_classification_loop_applies_the_stage_to_data_pt_batches_only(tmp_path, monkeypatch):
    from src.models.baselines import classification as S
    from src.models.biomedclip import classification as L
    monkeypatch.chdir(tmp_path)
    images, labels = _seg_blob(tmp_path / "seg.pt", S=64)
    blob = torch.load(tmp_path / "seg.pt")
    blob["labels"] = (labels.flatten(1).float().mean(1) > labels.float().mean()).long()
    torch.save(blob, tmp_path / "cls.pt")

    def train(argv, where):
        args = S.get_args(argv)
        args.train_snapshot_path = where
        torch.manual_seed(args.seed)
        return L.train(args, S.prepare_model)

    for out in _three_runs(train, ["--img_size", "64"], str(tmp_path / "cls.pt"), tmp_path):
        assert math.isfinite(out["last_loss"])


def test_clipseg_loop_applies_the_stage_to_data_pt_batches_only(tmp_path, monkeypatch):
    from src.models.clipseg import segmentation as S
    from src.third_party.openai_clip.model import CLIP
    monkeypatch.chdir(tmp_path)
    _seg_blob(tmp_path / "seg.pt", S=64)
    torch.manual_seed(2)
    torch.save(CLIP(64, 64, 10, 128, 16, 77, 49408, 64, 1, 2).state_dict(), tmp_path / "clip.pt")
    stats = tmp_path / "stats.json"

    def train(argv, where):
        args = S.get_args(argv + ["--stats_json", str(stats)])
        args.train_snapshot_path = where
        torch.manual_seed(args.seed)
        out = S.train(args)
        import json
        assert json.load(open(stats))["augmented_images"] == out["augmented_images"]
        return out

    _three_runs(train, ["--dataset", "BUSI", "--ckpt", str(tmp_path / "clip.pt"), "--img_size", "64"], str(tmp_path / "seg.pt"), tmp_path)
