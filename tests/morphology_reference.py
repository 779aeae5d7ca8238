"""The yardstick of uia_mask_morphology (csrc/morphology.hip), written from the contract in include/uia_hip.h and deliberately NOT through a distance
transform, so that it shares nothing with the kernel's formulation: a dilation is the union of the set shifted by every offset of the disk (offsets
with |dy| >= H or |dx| >= W are skipped: they move the whole image out of itself), an erosion goes through the complement inside the image, holes come
from an explicit-stack flood fill of the background, and the byte, overlay and statistics rules are applied with numpy.  tests/test_morphology_host.py
pins it on a literal mask and, where scipy imports, against scipy.ndimage."""
import numpy as np

INT_MAX = 2 ** 31 - 1


def disk_offsets(r):
    r = int(r)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def dilate(x, r):
    """x bool [H, W] -> {p in the image : some q in x with p - q in disk(r)}; nothing outside the image is set."""
    H, W = x.shape
    out = np.zeros_like(x)
    if not x.any():
        return out
    for k, (dy, dx) in enumerate(disk_offsets(r)):
        if abs(dy) >= H or abs(dx) >= W:
            continue
        if k % 64 == 0 and out.all():               # a union only grows: nothing is left to add
            break
        # out[y, x] |= x[y - dy, x - dx]
        ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
        xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        out[yd, xd] |= x[ys, xs]
    return out


def erode(x, r):
    """Only background inside the image erodes: the image minus the dilation of the in-image complement."""
    return ~dilate(~x, r)


def closing(x, r):
    return erode(dilate(x, r), r) if r > 0 else x.copy()


def opening(x, r):
    return dilate(erode(x, r), r) if r > 0 else x.copy()


def background_components(x, connectivity):
    """x bool [H, W] -> [(pixels as a list of raster indices, touches the frame)] for every connected component of ~x; explicit stack, no recursion."""
    H, W = x.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    seen = x.copy().ravel()                         # foreground counts as seen
    flat = seen.tolist()
    out = []
    for start in np.flatnonzero(~x.ravel()).tolist():
        if flat[start]:
            continue
        flat[start] = True
        stack, pixels, frame = [start], [], False
        while stack:
            p = stack.pop()
            pixels.append(p)
            y, xx = divmod(p, W)
            if y == 0 or xx == 0 or y == H - 1 or xx == W - 1:
                frame = True
            for dy, dx in steps:
                ny, nx = y + dy, xx + dx
                if 0 <= ny < H and 0 <= nx < W:
                    q = ny * W + nx
                    if not flat[q]:
                        flat[q] = True
                        stack.append(q)
        out.append((pixels, frame))
    return out


def filled_holes(x, hole_area, connectivity):
    """The pixels of the holes of x that are filled: background components that do not touch the frame, of any area (-1) or of at most hole_area."""
    fill = np.zeros(x.size, dtype=bool)
    if hole_area != 0:
        for pixels, frame in background_components(x, connectivity):
            if not frame and (hole_area < 0 or len(pixels) <= hole_area):
                fill[pixels] = True
    return fill.reshape(x.shape)


def transform(x0, r_close=0, r_open=0, hole_area=0, connectivity=4):
    """X0 -> X3, in the contract's order: closing, fill, opening."""
    x = closing(x0, int(r_close))
    x = x | filled_holes(x, int(hole_area), int(connectivity))
    return opening(x, int(r_open))


def apply(mask, overlay=None, r_close=0, r_open=0, hole_area=0, connectivity=4):
    """mask uint8 [H, W], overlay uint8 [H, W, 3] or None -> (mask after, overlay after or None, stats int32 [8])."""
    x0 = mask != 0
    x3 = transform(x0, r_close, r_open, hole_area, connectivity)
    new, gone = x3 & ~x0, x0 & ~x3
    out = mask.copy()
    out[new] = 255
    out[gone] = 0
    over = None
    if overlay is not None:
        over = overlay.copy()
        over[..., 1][new] = 255
        over[..., 1][gone] = overlay[..., 0][gone]
    ys, xs = np.nonzero(x3)
    box = [int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())] if ys.size else [INT_MAX, INT_MAX, -1, -1]
    stats = np.array([int(x3.sum())] + box + [int(new.sum()), int(gone.sum()), int(x0.sum())], dtype=np.int32)
    return out, over, stats


def overlay_of(mask, seed=0):
    """An overlay as uia_seg_predict_native writes it: (g, max(g, p), g) for a grey picture g and the mask p."""
    g = np.random.default_rng(seed).integers(0, 256, mask.shape, dtype=np.uint8)
    return np.stack([g, np.maximum(g, np.where(mask != 0, 255, 0).astype(np.uint8)), g], axis=-1)


def _ring(m, y0, x0, y1, x1, t=1):
    """The rim, t pixels thick, of the rectangle rows y0 .. y1, columns x0 .. x1 (inclusive); what lies outside the image is cut off, not moved in."""
    yy, xx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    inside = (yy >= y0) & (yy <= y1) & (xx >= x0) & (xx <= x1)
    core = (yy >= y0 + t) & (yy <= y1 - t) & (xx >= x0 + t) & (xx <= x1 - t)
    m[inside & ~core] = 255


def patterns(H, W, seed=0):
    """name -> uint8 [H, W]: the contents of the main sweep, scaled to the image and clipped where it is smaller than the figure."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    z = lambda: np.zeros((H, W), dtype=np.uint8)    # noqa: E731
    p = {"empty": z(), "full": np.full((H, W), 255, dtype=np.uint8)}
    m = z()
    m[H // 2, W // 2] = 255
    p["one_pixel"] = m
    yy, xx = np.mgrid[0:H, 0:W]
    p["checkerboard"] = (((yy + xx) % 2 == 0) * 255).astype(np.uint8)
    y0, x0, y1, x1 = H // 5 + 1, W // 5 + 1, H - H // 5 - 2, W - W // 5 - 2         # a rectangle that stays off the frame where the image allows one
    m = z()
    _ring(m, y0, x0, y1, x1, 2)
    p["ring"] = m
    m = z()
    _ring(m, -2, x0, y1, x1, 1)                     # its top rim lies outside the image: the inside reaches the first row and is no hole
    p["ring_on_frame"] = m
    m = z()
    _ring(m, y0, x0, y1, x1, 1)
    _ring(m, y0 + 3, x0 + 3, y1 - 3, x1 - 3, 1)
    p["ring_in_ring"] = m
    m = z()
    _ring(m, y0, x0, y1, x1, 1)
    if y1 > y0 and x1 > x0:
        m[y0, x0] = 0                               # the corner: the inside meets the outside only diagonally
    p["ring_diagonal_gap"] = m
    for gap in (1, 2, 5):
        m = z()
        _ring(m, y0, x0, y1, x1, 3)                 # three thick: the one-pixel tip of a disk reaches into the gap from either side, but not through it
        c = (x0 + x1) // 2
        if y1 > y0 and x1 > x0:
            m[y0:y0 + 3, max(c - gap // 2, 0):c - gap // 2 + gap] = 0
        p[f"ring_gap{gap}"] = m
    m = z()
    m[y0:H // 2 - 1, x0:x1 + 1] = 255
    m[H // 2 + 2:y1 + 1, x0:x1 + 1] = 255
    m[max(H // 2 - 1, 0):H // 2 + 2, W // 2] = 255                                   # the bridge between the two blobs: one pixel wide, three long (the
    #                                                                                  one-pixel tip of a disk restores the two ends, never the middle)
    p["bridge"] = m
    m = z()
    m[0:H // 3 + 1, 0:W // 2 + 1] = 255
    m[H - 1, W // 2:] = 255
    p["blob_on_frame"] = m
    for d in (0.3, 0.5, 0.7):
        p[f"noise{d}"] = ((rng.random((H, W)) < d) * 255).astype(np.uint8)
    v = p["ring_gap2"].copy()
    v[v != 0] = rng.integers(1, 255, int((v != 0).sum()), dtype=np.uint8)            # foreground bytes other than 255: they stay where the pixel stays
    p["values"] = v
    return p
