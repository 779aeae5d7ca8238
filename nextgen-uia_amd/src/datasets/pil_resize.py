"""Pillow's 8-bit resize restated in plain Python, one image at a time: the oracle of tests/test_resize_*.py and the written form of what
csrc/resize.hip (uia_resize_batch) computes.  The product path never calls it per batch.

`Image.resize` on an "L" or "RGB" image is the antialiased bicubic of Pillow's Resample.c; on a mode "1" mask it is the nearest scaler of Geometry.c.

Bicubic, per axis (in -> dst pixels), everything in float64, every product and every sum rounded on its own, sums in tap order:

    scale = in / dst; filterscale = max(scale, 1); support = 2 filterscale; ksize = 2 ceil(support) + 1; ss = 1 / filterscale
    output xx: center = (xx + 0.5) scale; xmin = max(0, int(center - support + 0.5)); xmax = min(in, int(center + support + 0.5)) - xmin
               w[x] = bicubic((x + xmin - center + 0.5) ss), a = -0.5, x < xmax; ww = w[0] + w[1] + ...; w[x] /= ww (ww != 0)
               k[x] = int(+-0.5 + w[x] 2^22), the sign of w[x]
    a pass:    clip8((2^21 + sum_x pixel[xmin + x] k[x]) >> 22) in integers

The horizontal pass runs first and leaves an 8-bit image, the vertical pass reads that; a pass whose axis keeps its size is skipped, and with both
skipped the bytes are copied.  Nearest: a = in / dst, xo = a / 2, output x reads source int(xo), xo += a — the coordinate is accumulated.
"""
import math

import numpy as np

PRECISION_BITS = 22
MAX_KSIZE = 129                                                 # the kernel's tap limit: a downscale of at most 32x


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def ksize_of(n_in, n_out):
    """Taps reserved per output pixel on an axis resampled from n_in to n_out pixels (the kernel takes at most MAX_KSIZE)."""
    filterscale = max(n_in / n_out, 1.0)
    return int(math.ceil(2.0 * filterscale)) * 2 + 1


def coefficients(n_in, n_out):
    """-> [(xmin, [k0, k1, ...])] per output pixel: the first source pixel and the 22-bit fixed-point weights."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:                                             # in tap order: np.sum would add pairwise
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out


def nearest_indices(n_in, n_out):
    a = n_in / n_out
    xo = a * 0.5
    idx = []
    for _ in range(n_out):
        idx.append(min(int(xo), n_in - 1))
        xo += a
    return idx


def _pass(src, coeffs, first, count):
    """One pass along axis 0 of an integer array [n_in, ...]: outputs first .. first + count - 1.  Integer arithmetic (exact in int64), taps in order."""
    out = np.empty((count,) + src.shape[1:], np.uint8)
    for o in range(count):
        xmin, k = coeffs[first + o]
        s = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t, kt in enumerate(k):
            s += src[xmin + t].astype(np.int64) * kt
        out[o] = np.clip(s >> PRECISION_BITS, 0, 255)
    return out


def resize_bicubic(pixels, dst_h, dst_w, window=None):
    """pixels: uint8 [H, W] or [H, W, C] -> the (y0, x0, h, w) window of the dst_h x dst_w resample, uint8 [h, w(, C)].  window None: the whole result."""
    pixels = np.asarray(pixels, np.uint8)
    H, W = pixels.shape[:2]
    y0, x0, h, w = window or (0, 0, dst_h, dst_w)
    if W != dst_w:
        mid = np.swapaxes(_pass(np.swapaxes(pixels, 0, 1), coefficients(W, dst_w), x0, w), 0, 1)
    else:
        mid = pixels[:, x0:x0 + w]
    if H == dst_h:
        return np.ascontiguousarray(mid[y0:y0 + h])
    return _pass(mid, coefficients(H, dst_h), y0, h)


def resize_nearest(pixels, dst_h, dst_w, window=None):
    """uint8 [H, W] (a mode "1" mask as Pillow holds it, one byte per pixel) -> the window of the nearest-neighbour resample."""
    pixels = np.asarray(pixels, np.uint8)
    H, W = pixels.shape
    y0, x0, h, w = window or (0, 0, dst_h, dst_w)
    ys, xs = nearest_indices(H, dst_h)[y0:y0 + h], nearest_indices(W, dst_w)[x0:x0 + w]
    return pixels[np.asarray(ys)[:, None], np.asarray(xs)[None, :]]
