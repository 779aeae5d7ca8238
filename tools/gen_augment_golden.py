#!/usr/bin/env python
"""Writes tests/golden/augment_cases.npz: small 8-bit images with masks, program tables (src/datasets/augment.py layout) and what PIL ITSELF makes of them —
the fixtures tests/test_augment_host.py holds the numpy restatement (tests/augment_reference.py) to, and through it the kernel (csrc/augment.hip).

Needs Pillow (12.2 wrote the committed file); nothing else of the reference's stack.  Every op is called the way the reference's dataset modules call it
(src/datasets/segmentation.py:14-153): ImageOps.autocontrast / equalize / posterize / solarize, ImageEnhance.Contrast / Brightness / Sharpness(...).enhance(v),
ImageFilter.GaussianBlur(radius=sigma), and for the weak ops torchvision's functional forms on PIL images.  torchvision is not needed: on a PIL image
F.resized_crop(img, i, j, h, w, size) IS img.crop((j, i, j + w, i + h)).resize(size[::-1], BILINEAR), F.hflip / F.vflip are img.transpose(FLIP_LEFT_RIGHT /
FLIP_TOP_BOTTOM), and a mode "1" mask is resized with NEAREST whatever filter is asked for (PIL forces it) — those calls are made here directly.

Per size S in (37, 64): in_S uint8 [3, S, S], mask_S uint8 [3, S, S] in {0, 1}, tab_S int32 [C, 14, 4], src_S int64 [C] (which image), out_S uint8
[C, S, S] and outmask_S uint8 [C, S, S] (PIL's results), name_S [C].  Cases whose name starts with "blur" hold PIL's three-pass box approximation: the
restatement's blur is the true Gaussian, and only its DISTANCE from PIL is recorded (DESIGN.md §4 "Augmentation").

    python tools/gen_augment_golden.py            # rewrites the file
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_reference as R  # noqa: E402  (opcodes and the table layout only: no pixel of the file comes from the restatement)

(IDENTITY, AUTOCONTRAST, EQUALIZE, BLUR, CONTRAST, BRIGHTNESS, SHARPNESS, POSTERIZE, SOLARIZE, CROP, HFLIP, VFLIP) = range(12)


def test_images(S, rng):
    """Three planes: a speckled 'ultrasound' fan (dark corners: many zeros), a low-contrast band of grey levels, and dense noise."""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    r = np.hypot(yy + 2, xx - S / 2)
    fan = (np.abs(xx - S / 2) < (yy + 3) * 0.8) & (r < S * 1.02)
    speckle = rng.gamma(2.0, 0.18, (S, S)) * (0.55 + 0.45 * np.sin(r / 3.1) * np.cos(xx / 5.3))
    a = np.clip(speckle * fan * 255, 0, 255).astype(np.uint8)
    b = (96 + 40 * np.sin(yy / 6.0 + xx / 9.0) + rng.integers(0, 12, (S, S))).astype(np.uint8)
    c = rng.integers(0, 256, (S, S)).astype(np.uint8)
    imgs = np.stack([a, b, c])
    cy, cx = S * 0.55, S * 0.45
    masks = np.stack([((yy - cy) / (S * 0.22)) ** 2 + ((xx - cx) / (S * 0.3)) ** 2 <= 1, (yy + xx) % 7 < 3, rng.random((S, S)) < 0.5]).astype(np.uint8)
    return imgs, masks


def pil_run(u, m, prog):
    """prog: rows (opcode, p0, p1, p2) with float parameters as Python floats of float32 values."""
    S = u.shape[0]
    img = Image.fromarray(u, "L")
    lab = Image.fromarray(m * 255, "L").convert("1")
    for code, p0, p1, p2 in prog:
        if code == AUTOCONTRAST:
            img = ImageOps.autocontrast(img)
        elif code == EQUALIZE:
            img = ImageOps.equalize(img)
        elif code == BLUR:
            img = img.filter(ImageFilter.GaussianBlur(radius=p0))
        elif code == CONTRAST:
            img = ImageEnhance.Contrast(img).enhance(p0)
        elif code == BRIGHTNESS:
            img = ImageEnhance.Brightness(img).enhance(p0)
        elif code == SHARPNESS:
            img = ImageEnhance.Sharpness(img).enhance(p0)
        elif code == POSTERIZE:
            img = ImageOps.posterize(img, p0)
        elif code == SOLARIZE:
            img = ImageOps.solarize(img, p0)
        elif code == CROP:
            i, j, side = p0, p1, p2
            img = img.crop((j, i, j + side, i + side)).resize((S, S), Image.BILINEAR)
            lab = lab.crop((j, i, j + side, i + side)).resize((S, S), Image.BILINEAR)
        elif code == HFLIP:
            img, lab = img.transpose(Image.FLIP_LEFT_RIGHT), lab.transpose(Image.FLIP_LEFT_RIGHT)
        elif code == VFLIP:
            img, lab = img.transpose(Image.FLIP_TOP_BOTTOM), lab.transpose(Image.FLIP_TOP_BOTTOM)
        elif code != IDENTITY:
            raise ValueError(code)
    return np.asarray(img).copy(), np.asarray(lab).astype(np.uint8)


def f32(v):
    return float(np.float32(v))


def cases(S):
    """(name, image index, program)."""
    lo = int(np.ceil(np.sqrt(0.8) * S))                        # the smallest side get_params can draw
    out = []
    for k in range(3):
        out += [(f"autocontrast_{k}", k, [(AUTOCONTRAST, 0, 0, 0)]), (f"equalize_{k}", k, [(EQUALIZE, 0, 0, 0)])]
        out += [(f"blur_{s}_{k}", k, [(BLUR, f32(s), 0, 0)]) for s in (0.75, 1.0, 1.25)]
    for n, v in enumerate((0.7500001, 0.9, 1.0, 1.1337, 1.25)):
        out += [(f"contrast_{n}", n % 3, [(CONTRAST, f32(v), 0, 0)]), (f"brightness_{n}", (n + 1) % 3, [(BRIGHTNESS, f32(v), 0, 0)]),
                (f"sharpness_{n}", (n + 2) % 3, [(SHARPNESS, f32(v), 0, 0)])]
    out += [(f"posterize_{bits}", bits % 3, [(POSTERIZE, bits, 0, 0)]) for bits in (4, 5, 6, 7)]
    out += [(f"solarize_{t}", t % 3, [(SOLARIZE, t, 0, 0)]) for t in (1, 77, 128, 255)]
    out += [("identity", 0, [(IDENTITY, 0, 0, 0)]), ("hflip", 0, [(HFLIP, 0, 0, 0)]), ("vflip", 1, [(VFLIP, 0, 0, 0)])]
    out += [("crop_whole", 0, [(CROP, 0, 0, S)]), ("crop_min_corner", 1, [(CROP, S - lo, S - lo, lo)]), ("crop_odd", 0, [(CROP, 1, 3, S - 4)]),
            ("crop_minus1", 2, [(CROP, 1, 0, S - 1)]), ("crop_mid", 2, [(CROP, 2, 1, (lo + S) // 2)])]
    # composed: the longest program the sampler can draw (9 strong + 4 weak), with repeated ops and two crops; no blur (PIL's is another filter)
    out.append(("composed13", 0, [(CONTRAST, f32(1.2), 0, 0), (AUTOCONTRAST, 0, 0, 0), (SHARPNESS, f32(0.8), 0, 0), (POSTERIZE, 6, 0, 0), (SHARPNESS, f32(1.25), 0, 0),
                                  (BRIGHTNESS, f32(0.9), 0, 0), (EQUALIZE, 0, 0, 0), (SOLARIZE, 200, 0, 0), (CONTRAST, f32(0.77), 0, 0),
                                  (CROP, 3, 1, S - 3), (HFLIP, 0, 0, 0), (CROP, 0, 2, S - 2), (VFLIP, 0, 0, 0)]))
    out.append(("composed_weak", 1, [(VFLIP, 0, 0, 0), (CROP, 2, 3, S - 3), (HFLIP, 0, 0, 0), (IDENTITY, 0, 0, 0)]))
    out.append(("composed_strong", 2, [(EQUALIZE, 0, 0, 0), (BRIGHTNESS, f32(1.25), 0, 0), (AUTOCONTRAST, 0, 0, 0), (SOLARIZE, 3, 0, 0), (POSTERIZE, 4, 0, 0),
                                       (CONTRAST, f32(1.25), 0, 0), (SHARPNESS, f32(1.0), 0, 0), (IDENTITY, 0, 0, 0), (EQUALIZE, 0, 0, 0)]))
    return out


def main():
    rng = np.random.default_rng(20240)
    blob = {}
    for S in (37, 64):
        imgs, masks = test_images(S, rng)
        cs = cases(S)
        tab = R.make_table([p for _, _, p in cs], with_mask=True)
        outs = [pil_run(imgs[k], masks[k], p) for _, k, p in cs]
        blob.update({f"in_{S}": imgs, f"mask_{S}": masks, f"tab_{S}": tab, f"src_{S}": np.array([k for _, k, _ in cs], dtype=np.int64),
                     f"out_{S}": np.stack([o[0] for o in outs]), f"outmask_{S}": np.stack([o[1] for o in outs]), f"name_{S}": np.array([n for n, _, _ in cs])})
    path = os.path.join(ROOT, "tests", "golden", "augment_cases.npz")
    np.savez_compressed(path, **blob)
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(len(cases(S)) for S in (37, 64))} cases")


if __name__ == "__main__":
    main()
