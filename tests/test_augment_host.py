"""CPU: the augmentation stage's host side.  The numpy restatement of the kernel (tests/augment_reference.py) against what PIL itself made of the
committed fixtures (tests/golden/augment_cases.npz, written by tools/gen_augment_golden.py) and against the installed PIL on fresh images; the blur's
recorded distance from PIL; the program sampler (src/datasets/augment.py); the argument checks of uia_augment_batch, which run before any GPU call."""
import ctypes
import functools
import os
import random
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import augment_reference as R  # noqa: E402
from src.datasets import augment as A  # noqa: E402

SIZES = (37, 64)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "augment_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_cases(S):
    z = golden()
    for c, name in enumerate(z[f"name_{S}"]):
        k, t = int(z[f"src_{S}"][c]), z[f"tab_{S}"][c]
        yield str(name), z[f"in_{S}"][k], z[f"mask_{S}"][k], t, z[f"out_{S}"][c], z[f"outmask_{S}"][c]


def test_opcodes_and_table_layout_agree_with_the_sampler():
    names = "IDENTITY AUTOCONTRAST EQUALIZE BLUR CONTRAST BRIGHTNESS SHARPNESS POSTERIZE SOLARIZE CROP HFLIP VFLIP MAX_OPS ROWS".split()
    assert [getattr(R, n) for n in names] == [getattr(A, n) for n in names]
    assert A.MAX_OPS == 13 and A.ROWS == 14 and len(A.STRONG_OPS) == 9 and len(A.WEAK_OPS) == 4
    from uia_hip import ops
    assert (ops.AUG_MAX_OPS, ops.AUG_ROWS) == (A.MAX_OPS, A.ROWS)
    assert R.f2i(1.25) == A.f32_bits(1.25) and R.f2i(0.8) == A.f32_bits(0.8)


@pytest.mark.parametrize("S", SIZES)
def test_restatement_equals_the_committed_pil_outputs(S):
    """Every op but the blur, alone and composed (a 13-op program with repeated ops and two crops among them): equal, pixel for pixel, image and mask."""
    seen = set()
    for name, u, m, t, want, want_m in golden_cases(S):
        got, got_m = R.run_program(u, m, t[1:1 + t[0, 0]])
        assert np.array_equal(got_m, want_m), f"{name}: mask differs from PIL in {(got_m != want_m).sum()} pixels"
        if not name.startswith("blur"):
            assert np.array_equal(got, want), f"{name}: {(got != want).sum()} pixels differ from PIL, max {np.abs(got.astype(int) - want.astype(int)).max()}"
        seen.update(int(c) for c in t[1:1 + t[0, 0], 0])
    assert seen == set(range(12))
    assert max(int(t[0, 0]) for _, _, _, t, _, _ in golden_cases(S)) == 13


def test_blur_distance_from_pil_is_the_one_design_md_records():
    """The blur is this build's (the true Gaussian), PIL's is a three-pass box approximation: DESIGN.md §4 "Augmentation" records the measured distance on
    the fixtures, and the restatement reproduces those figures.  Fewer than 1 % of the fixtures' pixels lie within 1e-3 of a rounding tie in float64 (the
    band in which the kernel's fp32 sum may round the other way)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = {(m.group(1), int(m.group(2))): (int(m.group(3)), float(m.group(4)))
            for m in re.finditer(r"^\| (blur_[\d.]+_\d) \| (\d+) \| (\d+) \| ([\d.]+) \|", text, flags=re.M)}
    n = 0
    for S in SIZES:
        for name, u, m, t, pil, _ in golden_cases(S):
            if not name.startswith("blur"):
                continue
            sigma = R.i2f(t[1, 1])
            d = np.abs(R.gaussian_blur(u, sigma).astype(int) - pil.astype(int))
            assert (name, S) in rows, f"DESIGN.md has no row for {name} at S = {S}"
            assert rows[(name, S)] == (int(d.max()), round(float(d.mean()), 3)), (name, S, int(d.max()), round(float(d.mean()), 3))
            ex = R.gaussian_blur_exact(u, sigma) + 0.5
            assert np.mean(np.abs(ex - np.round(ex)) < 1e-3) < 0.01
            n += 1
    assert n == 18 == len(rows)


def test_restatement_equals_the_installed_pil_on_fresh_images():
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    rng = np.random.default_rng(int(PIL.__version__.split(".")[0]))
    for S in (24, 37, 64, 85):
        for kind in range(3):
            u = (rng.integers(0, 256, (S, S)) if kind == 0 else rng.integers(90, 99, (S, S)) if kind == 1 else
                 np.clip(rng.gamma(2.0, 30.0, (S, S)) * (rng.random((S, S)) < 0.6), 0, 255)).astype(np.uint8)
            m = (rng.random((S, S)) < 0.5).astype(np.uint8)
            im, lab = Image.fromarray(u, "L"), Image.fromarray(m * 255, "L").convert("1")
            v = float(np.float32(rng.uniform(0.75, 1.25)))
            bits, thr = int(rng.integers(4, 8)), int(rng.integers(1, 256))
            side = int(rng.integers(int(np.ceil(np.sqrt(0.8) * S)), S + 1))
            i, j = int(rng.integers(0, S - side + 1)), int(rng.integers(0, S - side + 1))
            pairs = [(R.autocontrast(u), ImageOps.autocontrast(im)), (R.equalize(u), ImageOps.equalize(im)), (R.contrast(u, v), ImageEnhance.Contrast(im).enhance(v)),
                     (R.brightness(u, v), ImageEnhance.Brightness(im).enhance(v)), (R.sharpness(u, v), ImageEnhance.Sharpness(im).enhance(v)),
                     (R.smooth(u), im.filter(ImageFilter.SMOOTH)), (R.posterize(u, bits), ImageOps.posterize(im, bits)), (R.solarize(u, thr), ImageOps.solarize(im, thr)),
                     (R.crop_resize_bilinear(u, i, j, side), im.crop((j, i, j + side, i + side)).resize((S, S), Image.BILINEAR)),
                     (R.crop_resize_nearest(m, i, j, side), np.asarray(lab.crop((j, i, j + side, i + side)).resize((S, S), Image.BILINEAR)).astype(np.uint8))]
            for n, (got, want) in enumerate(pairs):
                assert np.array_equal(got, np.asarray(want)), (S, kind, n, v, bits, thr, (i, j, side))
    # the nearest scaler steps its source coordinate in float64: at S = 85, side = 80 it lands one ulp below the integers 40, 56, 72
    assert [int(v) for v in R.nearest_index(80, 85)[[42, 59, 76]]] == [39, 55, 71]
    lab = Image.fromarray((np.arange(80)[None, :].repeat(80, 0) % 2 * 255).astype(np.uint8), "L").convert("1")
    assert np.array_equal(np.asarray(lab.resize((85, 85), Image.BILINEAR)).astype(int)[0], R.nearest_index(80, 85) % 2)


def test_an_empty_program_returns_the_input_bits_and_a_program_quantises_once():
    rng = np.random.default_rng(3)
    x = rng.random((2, 1, 16, 16)).astype(np.float32)
    x[0, 0, 0, :4] = [np.nan, -0.0, 1.5, 1e-30]
    m = rng.integers(0, 256, (2, 1, 16, 16)).astype(np.uint8)
    t = R.make_table([[], [(R.IDENTITY, 0, 0, 0)]], with_mask=True)
    oi, om = R.augment_batch(x, m, t)
    assert np.array_equal(oi[0].view(np.int32), x[0].view(np.int32)) and np.array_equal(om, m)
    assert np.array_equal(oi[1, 0], R.quantise(x[1, 0]).astype(np.float32) / np.float32(255))
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantise(k.astype(np.float32) / np.float32(255)), k)


# ------------------------------------------------------------------------------------------------ the sampler
def _rows(table):
    for b in range(table.shape[0]):
        yield [tuple(int(v) for v in r) for r in table[b, 1:1 + table[b, 0, 0]]]


def test_sampler_counts_parameters_and_crops_stay_in_the_reference_ranges():
    S, B = 224, 4000
    t = A.draw_programs(B, S, True, True, True, A.make_rng(1, 0, 0, 0))
    assert t.shape == (B, 14, 4) and t.dtype == np.int32 and (t[:, 0, 1] == 1).all() and (t[:, 0, 2:] == 0).all()
    n = t[:, 0, 0]
    assert n.min() == 0 and n.max() <= 13
    # untouched: the coin (1/2) or both counts zero (1/2 · 1/10 · 1/5): p = 0.51; four standard deviations of a binomial of 4000 are 0.032
    assert abs(float((n == 0).mean()) - 0.51) < 0.032
    seen, lo_side = set(), int(round(np.sqrt(0.8) * S))
    for rows in _rows(t):
        codes = [r[0] for r in rows]
        # at most nine strong ops, then at most four weak ones (identity is in both lists: some split must fit)
        assert any(all(c in A.STRONG_OPS for c in codes[:k]) and all(c in A.WEAK_OPS for c in codes[k:]) and len(codes) - k <= 4 for k in range(min(9, len(codes)) + 1))
        for code, p0, p1, p2 in rows:
            seen.add(code)
            if code == A.BLUR:
                assert 0.75 <= R.i2f(p0) <= 1.25
            elif code in (A.CONTRAST, A.BRIGHTNESS, A.SHARPNESS):
                assert 0.75 <= R.i2f(p0) <= 1.25
            elif code == A.POSTERIZE:
                assert 4 <= p0 <= 7
            elif code == A.SOLARIZE:
                assert 1 <= p0 <= 255
            elif code == A.CROP:
                assert lo_side <= p2 <= S and 0 <= p0 <= S - p2 and 0 <= p1 <= S - p2
            if code not in (A.BLUR, A.CONTRAST, A.BRIGHTNESS, A.SHARPNESS, A.POSTERIZE, A.SOLARIZE, A.CROP):
                assert (p0, p1, p2) == (0, 0, 0)
            if code != A.CROP:
                assert (p1, p2) == (0, 0)
    assert seen == set(range(12))
    # the rows past a program's end stay zero
    assert all((t[b, 1 + n[b]:] == 0).all() for b in range(0, B, 97))


def test_sampler_one_flag_always_runs_and_none_never_does():
    S, B = 64, 2000
    s = A.draw_programs(B, S, True, False, False, A.make_rng(2))
    w = A.draw_programs(B, S, False, True, True, A.make_rng(2))
    z = A.draw_programs(B, S, False, False, True, A.make_rng(2))
    assert (z[:, 0, 0] == 0).all() and (s[:, 0, 1] == 0).all()
    assert abs(float((s[:, 0, 0] == 0).mean()) - 0.1) < 0.03 and s[:, 0, 0].max() == 9          # n = randint(0, 10): zero one time in ten
    assert abs(float((w[:, 0, 0] == 0).mean()) - 0.2) < 0.04 and w[:, 0, 0].max() == 4          # n = randint(0, 5)
    assert all(r[0] in A.STRONG_OPS for rows in _rows(s) for r in rows) and all(r[0] in A.WEAK_OPS for rows in _rows(w) for r in rows)
    assert abs(np.mean([r[0] == A.CROP for rows in _rows(w) for r in rows]) - 0.25) < 0.04        # choices with replacement, uniform over the four


def test_crop_fallback_is_taken_when_every_try_is_too_large():
    u = iter(np.random.default_rng(0).random(64).tolist()).__next__
    assert A.crop_params(64, u, scale=(1.01, 1.2)) == (0, 0, 64)
    t = A.draw_programs(500, 64, False, True, True, A.make_rng(5), crop_scale=(1.05, 1.2))
    crops = [r for rows in _rows(t) for r in rows if r[0] == A.CROP]
    assert len(crops) > 100 and all(r == (A.CROP, 0, 0, 64) for r in crops)
    # and a scale that always fits never takes it
    t = A.draw_programs(500, 64, False, True, True, A.make_rng(5), crop_scale=(0.8, 0.9))
    assert all(r[3] < 64 for rows in _rows(t) for r in rows if r[0] == A.CROP)


def test_sampler_is_seeded_by_its_own_generator_and_leaves_the_global_ones_alone():
    import torch
    random.seed(11)
    np.random.seed(12)
    torch.manual_seed(13)
    before = (random.getstate(), np.random.get_state(), torch.get_rng_state().clone())
    a = A.draw_programs(32, 224, True, True, True, A.make_rng(7, 1, 2, 3))
    b = A.draw_programs(32, 224, True, True, True, A.make_rng(7, 1, 2, 3))
    out = np.full((32, 14, 4), -1, dtype=np.int32)
    assert A.draw_programs(32, 224, True, True, True, A.make_rng(7, 1, 2, 3), out=out) is out
    assert np.array_equal(a, b) and np.array_equal(a, out)
    for other in ((8, 1, 2, 3), (7, 0, 2, 3), (7, 1, 3, 3), (7, 1, 2, 4)):
        assert not np.array_equal(a, A.draw_programs(32, 224, True, True, True, A.make_rng(*other)))
    after = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    assert before[0] == after[0] and torch.equal(before[2], after[2])
    assert before[1][0] == after[1][0] and np.array_equal(before[1][1], after[1][1]) and before[1][2:] == after[1][2:]


def test_stage_switch_follows_the_flags_and_the_data_source():
    import argparse
    ns = lambda **kw: argparse.Namespace(**{"strong_augs": True, "weak_augs": True, "data_pt": None, "synthetic": False, "seed": 4, **kw})
    assert A.stage_for(ns(synthetic=True), True) is None                                      # the noise images of timing runs and tests: never touched
    assert A.stage_for(ns(data_pt="d.pt", strong_augs=False, weak_augs=False), True) is None
    st = A.stage_for(ns(data_pt="d.pt", weak_augs=False), False, rank=3)
    assert (st.strong, st.weak, st.with_mask, st.seed, st.rank, st.augmented) == (True, False, False, 4, 3, 0)
    st.set_epoch(5)
    assert (st.epoch, st.iteration) == (5, 0)
    assert A.stage_for(argparse.Namespace(data_pt="d.pt"), True) is None                      # an entry point without the flags


# ------------------------------------------------------------------------------------------------ the C ABI's refusals (no GPU call is reached)
def test_uia_augment_batch_refuses_bad_arguments_before_touching_the_gpu():
    from uia_hip import _lib
    lib = _lib.lib()
    S, B = 16, 2
    assert lib.uia_augment_workspace_bytes(0, S) == 0 and lib.uia_augment_workspace_bytes(B, 7) == 0 and lib.uia_augment_workspace_bytes(B, 1025) == 0
    need = lib.uia_augment_workspace_bytes(B, S)
    assert need >= B * (14 * 16 + 8 * S * S)
    # host buffers stand in for device memory: every call below must return before any of them is touched
    img, out = np.zeros(B * S * S + 4, np.float32), np.zeros(B * S * S + 4, np.float32)
    msk, outm = np.zeros(B * S * S, np.uint8), np.zeros(B * S * S, np.uint8)
    ws = np.zeros(need + 16, np.uint8)
    wsp = (ws.ctypes.data + 15) & ~15
    good = R.make_table([[(R.CROP, 1, 2, 14)], []], with_mask=True)

    def call(tab=good, B=B, S=S, images=img.ctypes.data, masks=msk.ctypes.data, ws=wsp, ws_bytes=need, out_images=out.ctypes.data, out_masks=outm.ctypes.data):
        tab = None if tab is None else np.ascontiguousarray(tab, dtype=np.int32)
        rc = lib.uia_augment_batch(None, B, S, images, masks, None if tab is None else tab.ctypes.data, ws, ws_bytes, out_images, out_masks)
        return rc, lib.uia_last_error().decode()

    def tab_with(row, n=1):
        t = good.copy()
        t[0, 0, 0], t[0, 1] = n, row
        return t

    for what, kw, text in [("B = 0", dict(B=0), "bad shape"), ("S too small", dict(S=4), "bad shape"), ("null images", dict(images=None), "null"),
                           ("null table", dict(tab=None), "null"), ("null workspace", dict(ws=None), "null"), ("null output", dict(out_images=None), "null"),
                           ("mask without its output", dict(out_masks=None), "go together"), ("in place", dict(out_images=img.ctypes.data), "must not be the inputs"),
                           ("output one element into the input", dict(out_images=img.ctypes.data + 4), "overlap"),
                           ("output ending inside the input", dict(out_images=img.ctypes.data - 4 * (B * S * S - 1)), "overlap"),
                           ("mask output inside the mask", dict(out_masks=msk.ctypes.data + S * S), "overlap"),
                           ("misaligned workspace", dict(ws=wsp + 4), "aligned"), ("short workspace", dict(ws_bytes=need - 1), "needed"),
                           ("14 ops", dict(tab=tab_with((0, 0, 0, 0), n=14)), "ops"), ("negative count", dict(tab=tab_with((0, 0, 0, 0), n=-1)), "ops"),
                           ("unknown opcode", dict(tab=tab_with((12, 0, 0, 0))), "unknown opcode"), ("negative opcode", dict(tab=tab_with((-1, 0, 0, 0))), "unknown opcode"),
                           ("crop past the bottom", dict(tab=tab_with((R.CROP, 3, 0, 14))), "leaves"), ("crop past the right", dict(tab=tab_with((R.CROP, 0, 3, 14))), "leaves"),
                           ("crop larger than the image", dict(tab=tab_with((R.CROP, 0, 0, 17))), "leaves"), ("empty crop", dict(tab=tab_with((R.CROP, 0, 0, 0))), "leaves"),
                           ("negative corner", dict(tab=tab_with((R.CROP, -1, 0, 14))), "leaves"),
                           ("huge side", dict(tab=tab_with((R.CROP, 2**31 - 1, 0, 2**31 - 1))), "leaves"),
                           ("sigma 0", dict(tab=tab_with((R.BLUR, R.f2i(0.0), 0, 0))), "sigma"), ("sigma NaN", dict(tab=tab_with((R.BLUR, R.f2i(float("nan")), 0, 0))), "sigma"),
                           ("factor -1", dict(tab=tab_with((R.CONTRAST, R.f2i(-1.0), 0, 0))), "factor"), ("0 bits", dict(tab=tab_with((R.POSTERIZE, 0, 0, 0))), "posterize"),
                           ("threshold 300", dict(tab=tab_with((R.SOLARIZE, 300, 0, 0))), "solarize")]:
        rc, err = call(**kw)
        assert rc != 0 and text in err, (what, rc, err)
    assert not img.any() and not out.any() and not outm.any() and not ws.any()
    assert ctypes.sizeof(ctypes.c_int32) == 4
