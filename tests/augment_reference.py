"""Host restatement of the augmentation stage (csrc/augment.hip, uia_augment_batch) in numpy: every op on an 8-bit plane as PIL 12.2 computes it
(integer arithmetic, float32 where PIL's C code uses float, float64 where it uses double), and the interpreter of a per-image program table.

The only op that is NOT PIL's is the Gaussian blur: PIL's GaussianBlur is a three-pass box approximation; this build's is the true separable Gaussian of
the drawn sigma (taps out to ceil(4 sigma), replicated edges, rounded half up).  `gaussian_blur_exact` returns its float64 value before rounding, which
is what the kernel's fp32 accumulation is checked against.

Program table (int32 [B, 14, 4]): row 0 of an image is (n, with_mask, 0, 0), rows 1 .. n are (opcode, p0, p1, p2); float parameters are float32 bit
patterns.  Opcodes as in src/datasets/augment.py."""
import math

import numpy as np

IDENTITY, AUTOCONTRAST, EQUALIZE, BLUR, CONTRAST, BRIGHTNESS, SHARPNESS, POSTERIZE, SOLARIZE, CROP, HFLIP, VFLIP = range(12)
MAX_OPS = 13
ROWS = MAX_OPS + 1
PRECISION_BITS = 32 - 8 - 2


def f2i(v):
    """float -> the int32 holding its float32 bit pattern."""
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


def i2f(w):
    """int32 bit pattern -> float32."""
    return np.array([w], dtype=np.int32).view(np.float32)[0]


def quantise(x):
    """float32 plane in [0, 1] -> uint8: rint(x * 255) in float32 (exact for k / 255 sources), clamped, NaN -> 0."""
    v = np.rint(np.asarray(x, dtype=np.float32) * np.float32(255.0))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.uint8)


def dequantise(u):
    return u.astype(np.float32) / np.float32(255.0)


def histogram(u):
    return np.bincount(u.reshape(-1), minlength=256).astype(np.int64)


def autocontrast(u):
    h = histogram(u)
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return u.copy()
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    lut = np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], dtype=np.uint8)
    return lut[u]


def equalize(u):
    """ImageOps.equalize of the installed PIL: the step is (total - LAST NON-ZERO bin) // 255, the table the running sum n // step from n = step // 2 over
    ALL bins, and Image.point() clamps a table entry above 255 to 255 (small images reach it: the step is floored)."""
    h = histogram(u)
    nz = h[h > 0]
    if len(nz) <= 1:
        return u.copy()
    step = (int(nz.sum()) - int(nz[-1])) // 255
    if not step:
        return u.copy()
    n = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    lut = np.minimum(n // step, 255).astype(np.uint8)
    return lut[u]


def blend(d, x, v):
    """Image.blend(degenerate, image, v) on uint8 planes: float32 t = d + v * (x - d); <= 0 -> 0, >= 255 -> 255, else truncated."""
    v = np.float32(v)
    df, xf = d.astype(np.float32), x.astype(np.float32)
    t = df + v * (xf - df)
    out = np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), np.trunc(t)))
    return out.astype(np.uint8)


def brightness(u, v):
    return blend(np.zeros_like(u), u, v)


def contrast_mean(u):
    h = histogram(u)
    total, s = int(h.sum()), int((h * np.arange(256)).sum())
    return (2 * s + total) // (2 * total)                      # int(mean + 0.5)


def contrast(u, v):
    return blend(np.full_like(u, contrast_mean(u)), u, v)


def smooth(u):
    """ImageFilter.SMOOTH: [1 1 1; 1 5 1; 1 1 1] / 13, floor(acc + 0.5); border pixels copied.  acc + 0.5 is never within 1 / 26 of an integer, so the
    integer form is exact whatever the float order."""
    a = u.astype(np.int64)
    out = u.copy()
    if u.shape[0] < 3 or u.shape[1] < 3:
        return out
    acc = sum(a[1 + dy:a.shape[0] - 1 + dy, 1 + dx:a.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * a[1:-1, 1:-1]
    out[1:-1, 1:-1] = ((2 * acc + 13) // 26).astype(np.uint8)
    return out


def sharpness(u, v):
    return blend(smooth(u), u, v)


def posterize(u, bits):
    return u & np.uint8((~(2 ** (8 - int(bits)) - 1)) & 255)


def solarize(u, thr):
    return np.where(u < int(thr), u, 255 - u).astype(np.uint8)


def blur_radius(sigma):
    return int(math.ceil(4.0 * float(np.float32(sigma))))


def blur_weights(sigma):
    """float64 weights w[k], k = -r .. r, of the float32 sigma, normalised."""
    s = float(np.float32(sigma))
    r = blur_radius(s)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * s * s))
    return w / w.sum()


def gaussian_blur_exact(u, sigma):
    """The float64 value of the separable Gaussian (replicated edges) before rounding."""
    w = blur_weights(sigma)
    r = (len(w) - 1) // 2
    S0, S1 = u.shape
    a = u.astype(np.float64)
    idx1 = np.clip(np.arange(S1)[:, None] + np.arange(-r, r + 1)[None, :], 0, S1 - 1)
    t = (a[:, idx1] * w).sum(-1)
    idx0 = np.clip(np.arange(S0)[:, None] + np.arange(-r, r + 1)[None, :], 0, S0 - 1)
    return (t[idx0, :] * w[None, :, None]).sum(1)


def gaussian_blur(u, sigma):
    return np.clip(np.floor(gaussian_blur_exact(u, sigma) + 0.5), 0, 255).astype(np.uint8)


def bilinear_coeffs(in_size, out_size):
    """PIL's precompute_coeffs for the triangle filter, in_size <= out_size: per output index (first source index, 22-bit fixed-point taps)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    first, taps = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        k = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - a if a < 1.0 else 0.0)
        ww = sum(k)                                             # left to right, as the C loop
        if ww != 0.0:
            k = [v / ww for v in k]
        kk = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k]
        first.append(xmin)
        taps.append(kk)
    return first, taps


def _resample_rows(a, first, taps):
    """One pass along the last axis: out[.., d] = clip8((2^21 + sum p * k) >> 22)."""
    out = np.empty(a.shape[:-1] + (len(first),), dtype=np.uint8)
    a = a.astype(np.int64)
    for d, (x0, kk) in enumerate(zip(first, taps)):
        acc = np.full(a.shape[:-1], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t, k in enumerate(kk):
            acc = acc + a[..., x0 + t] * k
        out[..., d] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def crop_resize_bilinear(u, i, j, side):
    """img.crop((j, i, j + side, i + side)).resize((S, S), BILINEAR): horizontal pass first, uint8 intermediate."""
    S = u.shape[0]
    c = u[i:i + side, j:j + side]
    if side == S:
        return c.copy()
    first, taps = bilinear_coeffs(side, S)
    h = _resample_rows(c, first, taps)                          # [side, S]
    return _resample_rows(h.T, first, taps).T.copy()            # [S, S]


def nearest_index(side, S):
    """Source index of every destination index of PIL's nearest resize of a `side` crop to S: int(xo) with xo = a / 2 + a + a + ... ACCUMULATED in
    float64, a = side / S (PIL's affine scaler steps the source coordinate).  It is floor((d + 0.5) * side / S) except where that product is an integer,
    (2d + 1) * side = 2 * S * m: there the accumulated sum may stand one ulp below m and PIL takes m - 1 (S = 85, side = 80: d = 42, 59, 76)."""
    a = side / S
    xo, idx = a * 0.5, []
    for _ in range(S):
        idx.append(min(int(xo), side - 1))
        xo += a
    return np.array(idx, dtype=np.int64)


def crop_resize_nearest(m, i, j, side):
    S = m.shape[0]
    idx = nearest_index(side, S)
    return m[i:i + side, j:j + side][idx][:, idx].copy()


def apply_op(u, m, op):
    """One table row on the 8-bit image plane u and the mask m (or None)."""
    code, p0, p1, p2 = (int(v) for v in op)
    if code == IDENTITY:
        return u, m
    if code == AUTOCONTRAST:
        return autocontrast(u), m
    if code == EQUALIZE:
        return equalize(u), m
    if code == BLUR:
        return gaussian_blur(u, i2f(p0)), m
    if code == CONTRAST:
        return contrast(u, i2f(p0)), m
    if code == BRIGHTNESS:
        return brightness(u, i2f(p0)), m
    if code == SHARPNESS:
        return sharpness(u, i2f(p0)), m
    if code == POSTERIZE:
        return posterize(u, p0), m
    if code == SOLARIZE:
        return solarize(u, p0), m
    if code == CROP:
        return crop_resize_bilinear(u, p0, p1, p2), (None if m is None else crop_resize_nearest(m, p0, p1, p2))
    if code == HFLIP:
        return u[:, ::-1].copy(), (None if m is None else m[:, ::-1].copy())
    if code == VFLIP:
        return u[::-1].copy(), (None if m is None else m[::-1].copy())
    raise ValueError(f"unknown opcode {code}")


def run_program(u, m, rows):
    """rows: int [n, 4].  u uint8 [S, S], m uint8 [S, S] or None."""
    for op in rows:
        u, m = apply_op(u, m, op)
    return u, m


def augment_batch(images, masks, table):
    """images float32 [B, 1, S, S], masks uint8 [B, 1, S, S] or None, table int32 [B, 14, 4] -> (images, masks) as uia_augment_batch writes them: an
    empty program copies both bit for bit; otherwise the image is quantised once, run through its ops and written back as u8 / 255."""
    images = np.asarray(images, dtype=np.float32)
    out_i = images.copy()
    out_m = None if masks is None else np.asarray(masks, dtype=np.uint8).copy()
    for b in range(images.shape[0]):
        n = int(table[b, 0, 0])
        if n == 0:
            continue
        u, m = run_program(quantise(images[b, 0]), None if masks is None else out_m[b, 0].copy(), table[b, 1:1 + n])
        out_i[b, 0] = dequantise(u)
        if m is not None:
            out_m[b, 0] = m
    return out_i, out_m


def make_table(programs, with_mask=False):
    """programs: per image a list of (opcode, p0, p1, p2) with floats given as floats -> int32 [B, 14, 4]."""
    t = np.zeros((len(programs), ROWS, 4), dtype=np.int32)
    for b, prog in enumerate(programs):
        t[b, 0, 0], t[b, 0, 1] = len(prog), int(with_mask)
        for r, op in enumerate(prog):
            code = int(op[0])
            ps = list(op[1:]) + [0] * (4 - len(op))
            if code in (BLUR, CONTRAST, BRIGHTNESS, SHARPNESS):
                ps[0] = f2i(ps[0])
            t[b, 1 + r] = [code] + [int(p) for p in ps]
    return t
