"""-m gpu: uia_resize_batch_rgb (csrc/resize.hip) — gray and RGB images mixed in one launch, three planes out — against
src/datasets/pil_resize.resize_bicubic, which the host tests pin to Pillow; a gray result is replicated to the three planes (Pillow's convert("RGB")
of an "L" image followed by the resize).  ZERO differing values, compared as tests/test_resize_gpu.py compares.  The byte buffer starts one byte into
its allocation and the images lie back to back, so nothing is aligned; the output sits between NaN canaries."""
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

import resize_cases as RC  # noqa: E402
from guarded_out import Out, dev  # noqa: E402


def _img(name, W, H, C, S, kind="noise", geom=None):
    """One image with the loader's Resize(S) + CenterCrop(S) geometry (or `geom`: dst_h, dst_w, y0, x0)."""
    from src.datasets.captions import geometry
    dst_h, dst_w, y0, x0 = geom or geometry(W, H, S)
    c = dict(name=name, W=W, H=H, C=C, dst_w=dst_w, dst_h=dst_h, x0=x0, y0=y0, S=S, mask=False, kind=kind)
    return c, RC.make_input(c)[0]


# S = 16: an upscale; a landscape window at x0 = 4 (round(4.5) goes to even); a portrait; both passes skipped; a short side equal to S (both kept, a
# window at y0 = 12); one axis kept and one resampled; a smooth picture whose overshoot clips
MIXED16 = [_img("gray_up_9x8", 9, 8, 1, 16), _img("rgb_land_37x23", 37, 23, 3, 16), _img("rgb_port_23x37", 23, 37, 3, 16), _img("gray_keep_16x16", 16, 16, 1, 16),
           _img("rgb_16x40", 16, 40, 3, 16), _img("rgb_rows_kept_40x16", 40, 16, 3, 16, geom=(16, 25, 0, 4)), _img("rgb_smooth_64x48", 64, 48, 3, 16, "smooth")]
# S = 8: the 129-tap loop at exactly 32x (256 rows -> 8) on a gray image, beside an RGB image.  (The shorter-side rule would take the 300 columns
# to 9, which is 33x and beyond the kernel — the loader hands such a file to Pillow — so the columns go to 10 here, the window at x0 = 1.)
DEEP8 = [_img("gray_32x_300x256", 300, 256, 1, 8, geom=(8, 10, 0, 1)), _img("rgb_30x20", 30, 20, 3, 8)]
assert (MIXED16[1][0]["dst_w"], MIXED16[1][0]["x0"]) == (25, 4) and (MIXED16[0][0]["dst_w"], MIXED16[0][0]["dst_h"]) == (18, 16)


@pytest.fixture(scope="module")
def expected():
    """name -> uint8 [3, S, S] from the restated Pillow arithmetic, computed once."""
    from src.datasets.pil_resize import ksize_of, resize_bicubic
    out = {}
    for c, px in MIXED16 + DEEP8:
        r = resize_bicubic(px, c["dst_h"], c["dst_w"], RC.window_of(c))
        out[c["name"]] = np.repeat(r[None], 3, axis=0) if c["C"] == 1 else r.transpose(2, 0, 1).copy()
    assert ksize_of(256, 8) == 129
    smooth = out["rgb_smooth_64x48"]
    assert (smooth == 0).any() and (smooth == 255).any()        # the overshoot clips on both sides
    return out


def _pack(items):
    from src.datasets.folder import pack_ragged
    buf, desc = pack_ragged([(px, None, (c["dst_h"], c["dst_w"], c["y0"], c["x0"])) for c, px in items])
    desc[:, 3] = torch.tensor([c["C"] for c, _ in items], dtype=torch.int32)
    whole = torch.empty(buf.numel() + 1, dtype=torch.uint8, device=dev())
    whole[1:].copy_(buf)
    return whole[1:], desc


def _run(items):
    from uia_hip import ops
    S = items[0][0]["S"]
    src, desc = _pack(items)
    out = Out((len(items), 3, S, S), torch.float32)
    got = ops.resize_batch_rgb(src, desc, S, out.t)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.t.data_ptr() and out.intact(), "a canary around the output was overwritten"
    return src, desc, out.t


def _compare(items, images, expected):
    images = images.cpu()
    for b, (c, _) in enumerate(items):
        want = torch.from_numpy(expected[c["name"]])
        assert torch.equal(images[b], want.float() / 255), f"{c['name']}: {int((images[b] != want.float() / 255).sum())} values differ from Pillow's bytes / 255"
        assert int((torch.round(images[b] * 255).to(torch.uint8) != want).sum()) == 0, c["name"]


@pytest.mark.parametrize("items", [MIXED16, DEEP8], ids=["mixed16", "deep8"])
def test_mixed_batch_equals_pillow_in_every_value(items, expected):
    src, desc, images = _run(items)
    assert src.data_ptr() % 2 == 1 and {1, 3} == set(desc[:, 3].tolist())
    _compare(items, images, expected)


def test_single_images_and_two_calls_give_identical_bits(expected):
    from uia_hip import ops
    for item in (MIXED16[0], MIXED16[1], DEEP8[0]):             # B = 1 for each channel count, and the longest tap loop alone
        src, desc, images = _run([item])
        _compare([item], images, expected)
        again = ops.resize_batch_rgb(src, desc, item[0]["S"])
        assert torch.equal(again.view(torch.int32), images.view(torch.int32))
    src, desc, images = _run(MIXED16)
    assert torch.equal(ops.resize_batch_rgb(src, desc, 16).view(torch.int32), images.view(torch.int32))


def test_refusals_name_the_image_and_write_nothing():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    src, desc = _pack(MIXED16)
    out = Out((len(MIXED16), 3, 16, 16), torch.float32)

    def bad(row, col, value):
        d = desc.clone()
        d[row, col] = value
        return d

    with pytest.raises(UiaError, match="image 3 has 2 channels"):
        ops.resize_batch_rgb(src, bad(3, 3, 2), 16, out.t)
    with pytest.raises(UiaError, match="image 1.*window"):       # x0 = 10: 10 + 16 > 25
        ops.resize_batch_rgb(src, bad(1, 7, 10), 16, out.t)
    with pytest.raises(UiaError, match="image 5.*leaves the source buffer"):
        ops.resize_batch_rgb(src, bad(5, 0, src.numel() - 100), 16, out.t)
    with pytest.raises(UiaError, match="image 0.*leaves the source buffer"):     # a gray image declared RGB at the end of a short buffer
        ops.resize_batch_rgb(src[:72 * 2], bad(0, 3, 3)[:1], 16, out.t[:1])
    tall = torch.tensor([[0, 16, 16, 1, 16, 16, 0, 0], [0, 16 * 33, 1, 1, 16, 16, 0, 0]], dtype=torch.int32)
    with pytest.raises(UiaError, match="image 1.*32x"):          # a 33x downscale: 135 taps
        ops.resize_batch_rgb(torch.zeros(16 * 33, dtype=torch.uint8, device=dev()), tall, 16, out.t[:2])
    whole = torch.zeros(4 * 3 * 16 * 16 + 64, dtype=torch.uint8, device=dev())
    with pytest.raises(UiaError, match="overlap"):               # the output inside the source buffer
        ops.resize_batch_rgb(whole, tall[:1], 16, whole[:4 * 3 * 16 * 16].view(torch.float32).view(1, 3, 16, 16))
    with pytest.raises(UiaError):
        ops.resize_batch_rgb(src.cpu(), desc, 16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf).all())
