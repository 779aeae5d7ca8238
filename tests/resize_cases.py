"""The cases of tests/golden/resize_pil.npz, shared by tools/gen_resize_golden.py (which records Pillow's outputs) and tests/test_resize_*.py (which
regenerate the inputs and compare).  A case: name, source W x H, channels C, the size dst_w x dst_h it is resampled to, the window's corner (x0, y0),
the window's side S, whether it has a mask, and how its pixels are made ("noise": np.random.default_rng(seed) bytes; "smooth": a smooth image with
saturated blocks, so that the bicubic's negative lobes overshoot and clip8 clips on both sides)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pil.npz")


def _case(name, W, H, S, mask, kind="noise", C=1, dst=None, corner=(0, 0)):
    dst_w, dst_h = dst or (S, S)
    return dict(name=name, W=W, H=H, C=C, dst_w=dst_w, dst_h=dst_h, x0=corner[0], y0=corner[1], S=S, mask=mask, kind=kind)


# one list per (S, C): a list is one mixed batch of the GPU test
LISTS = {
    "L16": [_case("up_9x8", 9, 8, 16, True), _case("keep_16x16", 16, 16, 16, False), _case("down_100x90", 100, 90, 16, True),
            _case("smooth_50x70", 50, 70, 16, False, "smooth")],
    "L32": [_case("keep_32x32", 32, 32, 32, True), _case("taps129_37x1023", 37, 1023, 32, True), _case("down_64x47", 64, 47, 32, False),
            _case("smooth_90x40", 90, 40, 32, True, "smooth"), _case("rows_kept_33x32", 33, 32, 32, False)],
    "L224": [_case("cols_kept_224x300", 224, 300, 224, True), _case("near_225x223", 225, 223, 224, False), _case("down_471x562", 471, 562, 224, True),
             _case("smooth_600x448", 600, 448, 224, True, "smooth")],
    "RGB32": [_case("rgb_window_75x50", 75, 50, 32, False, C=3, dst=(48, 32), corner=(8, 0)),
              _case("rgb_window_40x90", 40, 90, 32, False, C=3, dst=(32, 72), corner=(0, 20)),
              _case("rgb_smooth_64x64", 64, 64, 32, False, "smooth", C=3)],
}
CASES = [c for cases in LISTS.values() for c in cases]


def seed_of(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"]))


def make_input(case):
    """-> (pixels uint8 [H, W] or [H, W, 3], mask bytes uint8 [H, W] in {0, 255} or None)."""
    H, W, C = case["H"], case["W"], case["C"]
    rng = np.random.default_rng(seed_of(case))
    if case["kind"] == "noise":
        px = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    else:
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        px = np.empty((H, W, C), np.uint8)
        for c in range(C):
            v = 127.5 + 127.5 * np.sin(xx * (0.31 + 0.05 * c)) * np.cos(yy * 0.17)
            v[H // 4:H // 2, W // 4:W // 2] = 255.0
            v[H // 2:3 * H // 4, W // 2:3 * W // 4] = 0.0
            px[..., c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    mask = (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255) if case["mask"] else None
    return (px[..., 0] if C == 1 else px), mask


def window_of(case):
    return (case["y0"], case["x0"], case["S"], case["S"])


def load_golden():
    """-> (expected {name: (image uint8 [S, S(, 3)], mask uint8 [S, S] in {0, 1} or None)}, the Pillow version that wrote them)."""
    z = np.load(GOLDEN)
    recorded = json.loads(str(z["cases"]))
    assert recorded == CASES, "tests/golden/resize_pil.npz was recorded for another case list: run tools/gen_resize_golden.py"
    return {c["name"]: (z["img_" + c["name"]], z["mask_" + c["name"]] if c["mask"] else None) for c in CASES}, str(z["pil_version"])
