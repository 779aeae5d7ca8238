"""-m gpu: uia_resize_batch (csrc/resize.hip) against tests/golden/resize_pil.npz, what Pillow's Image.resize gives, with ZERO differing bytes.  Each
list of tests/resize_cases.py is one mixed batch (sizes differ, so every image but the first starts at an unaligned offset; the buffer itself starts one
byte into its allocation): an upscale, axes that keep their size, both kept, the longest tap loop (ksize 129), smooth images that clip, RGB windows,
images with and without masks side by side, and B = 1.  The outputs sit between NaN / 0xA5 canaries."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "nextgen-uia_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resize_cases as RC  # noqa: E402
from guarded_out import dev  # noqa: E402

GUARD = 64


class Guarded:
    """A device tensor GUARD elements inside a sentinel-filled buffer."""

    def __init__(self, shape, dtype):
        self.n = math.prod(shape)
        self.sentinel = float("nan") if dtype == torch.float32 else 0xA5
        self.buf = torch.full((GUARD + self.n + GUARD,), self.sentinel, dtype=dtype, device=dev())
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)

    def untouched(self):
        b = self.buf.cpu()
        return all(bool(torch.isnan(p).all()) if self.sentinel != self.sentinel else bool((p == self.sentinel).all()) for p in (b[:GUARD], b[GUARD + self.n:]))


def _pack(cases):
    """-> (device byte buffer starting at an odd address, host descriptor): images and masks back to back, nothing aligned."""
    from src.datasets.folder import pack_ragged
    items = []
    for c in cases:
        px, mask = RC.make_input(c)
        items.append((px, mask, (c["dst_h"], c["dst_w"], c["y0"], c["x0"])))
    buf, desc = pack_ragged(items)
    whole = torch.empty(buf.numel() + 1, dtype=torch.uint8, device=dev())
    whole[1:].copy_(buf)
    return whole[1:], desc


def _run(cases):
    from uia_hip import ops
    S, C, B = cases[0]["S"], cases[0]["C"], len(cases)
    src, desc = _pack(cases)
    with_masks = any(c["mask"] for c in cases)
    oi = Guarded((B, C, S, S), torch.float32)
    om = Guarded((B, 1, S, S), torch.uint8) if with_masks else None
    got_i, got_m = ops.resize_batch(src, desc, S, C, oi.t, None if om is None else om.t)
    torch.cuda.synchronize()
    assert got_i.data_ptr() == oi.t.data_ptr() and (got_m is None) == (om is None)
    assert oi.untouched() and (om is None or om.untouched()), "a canary around the outputs was overwritten"
    return src, desc, oi.t, None if om is None else om.t


@pytest.fixture(scope="module")
def pil_golden():
    return RC.load_golden()[0]


def _compare(cases, images, masks, golden):
    S, C = cases[0]["S"], cases[0]["C"]
    images, masks = images.cpu(), None if masks is None else masks.cpu()
    for b, c in enumerate(cases):
        want_i, want_m = golden[c["name"]]
        want = torch.from_numpy(want_i.reshape(S, S, C).transpose(2, 0, 1).copy())
        assert torch.equal(images[b], want.float() / 255), f"{c['name']}: {int((images[b] != want.float() / 255).sum())} values differ from Pillow's bytes / 255"
        back = torch.round(images[b] * 255).to(torch.uint8)
        assert int((back != want).sum()) == 0, c["name"]
        if masks is not None:
            expect = torch.from_numpy(want_m) if want_m is not None else torch.zeros(S, S, dtype=torch.uint8)      # no mask in a batch with masks: zeros
            assert torch.equal(masks[b, 0], expect), f"{c['name']}: {int((masks[b, 0] != expect).sum())} mask bytes differ"


@pytest.mark.parametrize("which", list(RC.LISTS))
def test_mixed_batch_equals_pillow_in_every_byte(which, pil_golden):
    cases = RC.LISTS[which]
    assert len({(c["S"], c["C"]) for c in cases}) == 1
    src, desc, images, masks = _run(cases)
    assert any(int(o) % 4 for o in desc[:, 0].tolist()) or src.data_ptr() % 2 == 1
    _compare(cases, images, masks, pil_golden)


def test_single_image_batches_and_two_calls_give_identical_bits(pil_golden):
    from uia_hip import ops
    for c in (RC.LISTS["L32"][1], RC.LISTS["L16"][0], RC.LISTS["RGB32"][0]):      # the 129-tap case with its mask, the upscale, an RGB window
        src, desc, images, masks = _run([c])
        _compare([c], images, masks, pil_golden)
        again_i, again_m = ops.resize_batch(src, desc, c["S"], c["C"])
        assert torch.equal(again_i.view(torch.int32), images.view(torch.int32)) and (masks is None or torch.equal(again_m, masks))


def test_refusals_name_the_image_and_write_nothing():
    from uia_hip import ops
    from uia_hip._lib import UiaError
    cases = RC.LISTS["L16"]
    src, desc = _pack(cases)
    oi = Guarded((len(cases), 1, 16, 16), torch.float32)
    om = Guarded((len(cases), 1, 16, 16), torch.uint8)
    tall = torch.tensor([[0, 16, 16, -1, 16, 16, 0, 0], [0, 16, 16, -1, 16, 16, 0, 0], [0, 16 * 33, 1, -1, 16, 16, 0, 0]], dtype=torch.int32)
    with pytest.raises(UiaError, match="image 2"):              # a 33x downscale: 135 taps
        ops.resize_batch(torch.zeros(16 * 33, dtype=torch.uint8, device=dev()), tall, 16, 1, oi.t[:3])
    bad = desc.clone()
    bad[1, 6] = 1                                               # the window leaves dst
    with pytest.raises(UiaError, match="image 1"):
        ops.resize_batch(src, bad, 16, 1, oi.t, om.t)
    with pytest.raises(UiaError):
        ops.resize_batch(src.cpu(), desc, 16, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(oi.buf).all()) and bool((om.buf == 0xA5).all())
