"""Outputs that show a stray write: views at an offset inside NaN-filled device buffers, with guard elements on both sides.  A plain module,
no pytest: the contract tests of the small kernels (tests/test_helpers_contract_gpu.py) and of the UNet kernels
(tests/test_unet_contract_gpu.py) hand these to the kernels.  An element the kernel does not write stays NaN and fails its comparison;
a write outside the view (the guard regions, the padding columns of a strided view) fails the test."""
import math

import torch

PAD = 64                    # guard elements on each side of an output: keeps 128-byte (bf16) / 256-byte (fp32) alignment


def dev():
    return torch.device("cuda:0")


class Out:
    """A [rows, cols] (or `shape`) output view at offset PAD of a NaN-filled buffer, rows ld apart; `init` fills the view."""

    def __init__(self, shape, dt, ld=None, init=None, offset=PAD):
        shape = tuple(shape)
        cols = shape[-1]
        rows = math.prod(shape[:-1])
        self.ld, self.cols, self.rows, self.offset = ld or cols, cols, rows, offset
        self.buf = torch.full((offset + rows * self.ld + PAD,), float("nan"), dtype=dt, device=dev())
        body = self.buf[offset:offset + rows * self.ld].view(rows, self.ld)
        self.t = body[:, :cols] if self.ld != cols else body.view(shape)
        if init is not None:
            self.t.copy_(init.reshape(self.t.shape).to(dt))

    def intact(self):
        b = self.buf.cpu()
        ok = bool(torch.isnan(b[:self.offset]).all()) and bool(torch.isnan(b[self.offset + self.rows * self.ld:]).all())
        if self.ld != self.cols:
            ok &= bool(torch.isnan(b[self.offset:self.offset + self.rows * self.ld].view(self.rows, self.ld)[:, self.cols:]).all())
        return ok


def guards(ck, bar, ctx, *outs):
    for o in outs:
        if not o.intact():
            ck.fail(bar, ctx, "a write outside the output (guard region or padding columns)")
