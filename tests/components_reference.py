"""The yardstick of uia_mask_components (csrc/components.hip): a plain explicit-stack flood fill on the host, then the contract of include/uia_hip.h applied
with numpy — filter by area and rank, rewrite mask and overlay, statistics and the lesion list.  Everything is integer; comparisons are exact equality.
Shared by tests/test_components_host.py (which pins it, against scipy.ndimage.label where scipy imports) and tests/test_components_gpu.py."""
import numpy as np

INT_MAX = 2 ** 31 - 1
EMPTY_BOX = (INT_MAX, INT_MAX, -1, -1)


def flood_label(mask, connectivity):
    """mask [H, W] (non-zero = foreground) -> (labels int32 [H, W], 0 = background, components numbered from 1 in the order of their first pixel in raster
    order; n).  Explicit stack, one pixel at a time, over a flat array padded by one background pixel all round."""
    assert connectivity in (4, 8)
    fg = np.asarray(mask) != 0
    H, W = fg.shape
    P = W + 2
    flat = np.zeros((H + 2) * P, dtype=np.int8)
    flat.reshape(H + 2, P)[1:-1, 1:-1] = fg
    todo = flat.tolist()                            # 1 = foreground not yet labelled
    out = [0] * len(todo)
    steps = (-1, 1, -P, P) if connectivity == 4 else (-1, 1, -P, P, -P - 1, -P + 1, P - 1, P + 1)
    n = 0
    for start in np.flatnonzero(flat).tolist():     # raster order: a component's number follows its first pixel
        if not todo[start]:
            continue
        n += 1
        todo[start] = 0
        out[start] = n
        stack = [start]
        while stack:
            at = stack.pop()
            for s in steps:
                q = at + s
                if todo[q]:
                    todo[q] = 0
                    out[q] = n
                    stack.append(q)
    labels = np.asarray(out, dtype=np.int32).reshape(H + 2, P)[1:-1, 1:-1]
    return np.ascontiguousarray(labels), n


def components(labels, n):
    """-> per component (1-based number - 1): area, first pixel, ymin, xmin, ymax, xmax, sum y, sum x as int64 arrays, and `order`, the component indices
    sorted by (area descending, first pixel ascending)."""
    H, W = labels.shape
    flat = labels.ravel()
    idx = np.flatnonzero(flat)
    lab = flat[idx].astype(np.int64) - 1
    ys, xs = idx // W, idx % W
    area = np.bincount(lab, minlength=n).astype(np.int64)
    first = np.full(n, H * W, dtype=np.int64)
    np.minimum.at(first, lab, idx)
    ymin, xmin = np.full(n, INT_MAX, dtype=np.int64), np.full(n, INT_MAX, dtype=np.int64)
    ymax, xmax = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    np.minimum.at(ymin, lab, ys)
    np.minimum.at(xmin, lab, xs)
    np.maximum.at(ymax, lab, ys)
    np.maximum.at(xmax, lab, xs)
    sy = np.zeros(n, dtype=np.int64)
    sx = np.zeros(n, dtype=np.int64)
    np.add.at(sy, lab, ys)
    np.add.at(sx, lab, xs)
    order = np.lexsort((first, -area))
    return dict(area=area, first=first, ymin=ymin, xmin=xmin, ymax=ymax, xmax=xmax, sy=sy, sx=sx, order=order)


class Labelled:
    """A mask labelled once per connectivity; `apply` may then be called with any parameters."""

    def __init__(self, mask):
        self.mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self._by_conn = {}

    def parts(self, connectivity):
        if connectivity not in self._by_conn:
            labels, n = flood_label(self.mask, connectivity)
            self._by_conn[connectivity] = (labels, n, components(labels, n))
        return self._by_conn[connectivity]

    def apply(self, overlay=None, min_area=0, keep=0, connectivity=8, max_list=0):
        """-> (mask after, overlay after or None, stats int32 [8], list int32 [max_list, 8]) per the contract."""
        labels, n, c = self.parts(connectivity)
        order = c["order"]
        kept_sorted = c["area"][order] >= min_area
        if keep > 0:
            kept_sorted &= np.arange(n) < keep
        kept = np.zeros(n + 1, dtype=bool)          # by label; background is "not kept" but is never foreground either
        kept[order[kept_sorted] + 1] = True
        drop = (labels > 0) & ~kept[labels]
        mask = self.mask.copy()
        mask[drop] = 0
        over = None
        if overlay is not None:
            over = np.array(overlay, dtype=np.uint8, copy=True)
            over[..., 1][drop] = over[..., 0][drop]
        ys, xs = np.nonzero((labels > 0) & kept[labels])
        box = (int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())) if ys.size else EMPTY_BOX
        stats = np.array([ys.size, *box, n, int(kept_sorted.sum()), int((labels > 0).sum())], dtype=np.int32)
        rows = np.zeros((max_list, 8), dtype=np.int32)
        for k, i in enumerate(order[kept_sorted][:max_list]):
            a = int(c["area"][i])
            rows[k] = (a, c["ymin"][i], c["xmin"][i], c["ymax"][i], c["xmax"][i], c["first"][i], int(c["sy"][i]) // a, int(c["sx"][i]) // a)
        return mask, over, stats, rows


def apply(mask, overlay=None, min_area=0, keep=0, connectivity=8, max_list=0):
    return Labelled(mask).apply(overlay, min_area, keep, connectivity, max_list)


# ------------------------------------------------------------------------------------------------ the patterns of the tests
def spiral(H, W):
    """A one-pixel-wide path from the top-left corner inwards, clockwise, its arms one pixel apart: ONE component under both connectivities, and the
    longest walk through an image that a labelling can be asked to follow."""
    m = np.zeros((H, W), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        free = 0 <= ny < H and 0 <= nx < W and m[ny, nx] == 0 and not (0 <= fy < H and 0 <= fx < W and m[fy, fx])
        if free:
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1      # turn right; two turns without a step: the centre is reached
    return m


def patterns(H, W):
    """name -> uint8 [H, W] mask, non-zero = foreground (255 unless the pattern says otherwise)."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    out["checkerboard"] = (((yy + xx) % 2 == 0) * 255).astype(np.uint8)
    out["spiral"] = spiral(H, W) * np.uint8(255)
    comb = np.zeros((H, W), np.uint8)               # a spine along the top row, teeth on every second column
    comb[0, :] = 255
    comb[:, ::2] = 255
    out["comb"] = comb
    ring = np.maximum(np.abs(yy - H // 2), np.abs(xx - W // 2))
    out["rings"] = ((ring % 3 == 0) * 255).astype(np.uint8)
    corner = np.zeros((H, W), np.uint8)             # two blobs that touch only diagonally, at the corner of the first tile where the image has one
    cy, cx = (32 if H > 32 else max(1, H // 2)), (64 if W > 64 else max(1, W // 2))
    corner[max(0, cy - 5):cy, max(0, cx - 7):cx] = 255
    corner[cy:cy + 4, cx:cx + 6] = 255
    out["corner"] = corner
    for density, seed in ((0.3, 3), (0.5, 5), (0.6, 6)):
        out[f"random{density}"] = ((np.random.default_rng(seed).random((H, W)) < density) * 255).astype(np.uint8)
    values = np.random.default_rng(9).integers(1, 255, size=(H, W), dtype=np.uint8)          # non-zero bytes other than 255: kept pixels must keep them
    out["values"] = np.where(np.random.default_rng(10).random((H, W)) < 0.45, values, 0).astype(np.uint8)
    return out
