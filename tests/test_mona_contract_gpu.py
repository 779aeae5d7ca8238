"""-m gpu: what the Mona spatial kernels and the plain pre-norm kernels of csrc/mona.hip must compute, element by element against the float64
restatements of tests/mona_reference.py on the operands the kernel sees, at the grids, widths and row counts where the launcher or a kernel
changes behaviour (the tables of that module, chosen by its restatement of the launcher's formulas).

Every output, gradient buffer and workspace is a view inside a NaN-filled buffer with guard elements on both sides (tests/guarded_out.py), so the
calls go to the C entry points; each case also runs through its uia_hip.ops wrapper, whose d, dt, u, dx32 and dxT must be bit-identical.  Gradient
buffers always start from non-zero values: the result is prefill + gradient.  Each test loops over its cases and fails once with the collected
list (bar, case, worst flat index, error/bound); the bounds are counted in mona_reference, none is fitted to what a kernel returns."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import helpers_reference as R
import mona_reference as MR
from guarded_out import Out, dev, guards

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = (BF16, F32)
DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mona_perpixel_driver.py")


@pytest.fixture(scope="module")
def ops():
    from uia_hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from uia_hip import _lib
    return _lib.lib()


def up(t, dt=None):
    return None if t is None else t.to(dt if dt is not None else t.dtype).to(dev()).contiguous()


def p(t):
    return None if t is None else (t.t if isinstance(t, Out) else t).data_ptr()


def last_error():
    from uia_hip import _lib
    return _lib.lib().uia_last_error().decode()


def call(ck, ctx, name, rc):
    if rc != 0:
        ck.fail(name, ctx, f"rc={rc}: {last_error()}")
    return rc == 0


def finish(ck):
    assert ck.ok(), ck.report()
    print(ck.report())


def bar(name, dt):
    return name + (" bf16" if dt == BF16 else " fp32")


def kernel_tag(fast):
    return "fast" if fast else "per-pixel"


def prefill(n, seed):
    return MR.rnd(n, seed=7000 + seed, scale=0.5)


# ------------------------------------------------------------------------------------------ spatial
class Spatial:
    """The device operands of one case and its guarded launches."""

    def __init__(self, lib, ops, case):
        self.lib, self.ops, self.case = lib, ops, case
        self.t, self.dd, self.P, self.keep = MR.case_inputs(case)
        self.td, self.ddd = up(self.t), up(self.dd)
        self.Pd = {k: up(v) for k, v in self.P.items()}
        self.kd = up(self.keep)
        self.ntok = 1 + case.h * case.w
        self.ctx = MR.case_name(case)

    def desc(self):
        c = self.case
        return self.ops._spatial_desc(c.variant, c.B, c.h, c.w, self.td, self.Pd, c.p, 0, self.kd)

    def fwd(self):
        c = self.case
        d = Out((c.B, self.ntok, 64), c.dtype)
        q = self.desc()
        q.d = p(d)
        return self.lib.uia_mona_spatial_fwd(self.ops._stream(), self.ops._code(c.dtype), C.byref(q)), d

    def grad_buffers(self):
        return {k: Out((self.P[k].numel(),), F32, init=prefill(self.P[k].numel(), i)) for i, k in enumerate(MR.keys_of(self.case.variant))}

    def bwd(self, workspace=True):
        c = self.case
        dt, grads = Out((c.B, self.ntok, 64), c.dtype), self.grad_buffers()
        ws = Out((self.lib.uia_mona_spatial_workspace_bytes(c.B) // 4,), F32) if workspace else None
        q = self.desc()
        q.dd, q.dt, q.ws = p(self.ddd), p(dt), p(ws)
        for k, g in grads.items():
            setattr(q, "g_" + k, p(g))
        return self.lib.uia_mona_spatial_bwd(self.ops._stream(), self.ops._code(c.dtype), C.byref(q)), dt, grads, ws


def check_spatial(lib, ops, ck, case, fast_allowed=True, workspace=True, wrapper=True, backward=True, twice=False):
    """Forward and backward of one case against the restatement; `twice`: a second identical backward must return the same bits."""
    s = Spatial(lib, ops, case)
    ctx, dt = s.ctx, case.dtype
    fast = fast_allowed and MR.fast_path(dt, case.h, case.w, False)
    ref = MR.spatial_fwd(case.variant, s.t, s.P, case.h, case.w, s.keep, case.p)["d"]
    rc, d = s.fwd()
    if call(ck, ctx, "uia_mona_spatial_fwd", rc):
        ck.check(bar(f"spatial fwd d ({kernel_tag(fast)})", dt), d.t, ref.ref, MR.bound(ref, 1, dt, fast), ctx)
        guards(ck, "guards", ctx, d)
        if wrapper:
            d2 = torch.full((case.B, s.ntok, 64), float("nan"), dtype=dt, device=dev())
            ops.mona_spatial_fwd(case.variant, case.B, case.h, case.w, s.td, s.Pd, d2, p_drop=case.p, keep_mask=s.kd)
            ck.exact("wrapper d", d2, d.t, ctx)
    if not backward:
        return
    fast = fast_allowed and MR.fast_path(dt, case.h, case.w, True)
    tag = kernel_tag(fast) + ("" if workspace else ", atomic")
    refs = MR.spatial_bwd(case.variant, s.t, s.dd, s.P, case.h, case.w, s.keep, case.p)
    rc, dto, grads, ws = s.bwd(workspace)
    if not call(ck, ctx, "uia_mona_spatial_bwd", rc):
        return
    ck.check(bar(f"spatial bwd dt ({tag})", dt), dto.t, refs["dt"].ref, MR.bound(refs["dt"], 1, dt, fast), ctx)
    for i, (k, g) in enumerate(grads.items()):
        pre = prefill(s.P[k].numel(), i).reshape(s.P[k].shape)
        term = refs["g_" + k]
        ck.check(f"spatial bwd g_{k} ({tag})", g.t, term.ref + pre.to(torch.float64), MR.bound(term, 1, F32, fast, prefill=pre), ctx)
    guards(ck, "guards", ctx, dto, *grads.values(), *([ws] if ws else []))
    if twice:
        rc, dto2, grads2, ws2 = s.bwd(workspace)
        if call(ck, ctx, "uia_mona_spatial_bwd", rc):
            ck.exact("image sum in a fixed order: dt", dto2.t, dto.t, ctx)
            for k in grads:
                ck.exact(f"image sum in a fixed order: g_{k}", grads2[k].t, grads[k].t, ctx)
    if wrapper:
        dt2 = torch.full((case.B, s.ntok, 64), float("nan"), dtype=dt, device=dev())
        g2 = {k: up(prefill(s.P[k].numel(), i).reshape(s.P[k].shape)) for i, k in enumerate(grads)}
        ops.mona_spatial_bwd(case.variant, case.B, case.h, case.w, s.td, s.Pd, s.ddd, dt2, g2, p_drop=case.p, keep_mask=s.kd)
        ck.exact("wrapper dt", dt2, dto.t, ctx)


def test_spatial_per_pixel_kernel_bf16(lib, ops):
    ck = R.Checker()
    for case in MR.PIXEL_CASES:
        if case.dtype == BF16:
            check_spatial(lib, ops, ck, case)
    finish(ck)


def test_spatial_per_pixel_kernel_fp32(lib, ops):
    ck = R.Checker()
    for case in MR.PIXEL_CASES:
        if case.dtype == F32:
            check_spatial(lib, ops, ck, case)
    finish(ck)


def test_spatial_fast_kernel_width_4(lib, ops):
    """The zero-projector cases at 1 × 4 and 3 × 4 (two images) are the ones that found the weight gradient of the projector out: with nothing but its own
    matrix-core product in its bound, a sum of 8 and of 24 products of operands each rounded once to bf16 (up to 2^-8 of a value, bf16 keeping 8
    significant bits) stood at 1.18 and 1.16 of u_mfma·Σ|dz||c| (index 1015: 2.35324 for 2.33525; index 1578: −0.589026 for −0.599207), exactly the sum of the
    products of the rounded operands.  The dP phase of the fast kernel now feeds each operand as a hi + lo pair of bf16 values."""
    ck = R.Checker()
    for case in MR.FAST4_CASES:
        check_spatial(lib, ops, ck, case)
    finish(ck)


def test_spatial_fast_kernel_width_14(lib, ops):
    ck = R.Checker()
    for case in MR.FAST14_CASES:
        check_spatial(lib, ops, ck, case)
    finish(ck)


def test_spatial_fall_back_and_largest_grids(lib, ops):
    """The last grid of the fast kernel, the first and the last of the per-pixel kernel behind it, in each direction (mona_reference.limit_grids)."""
    ck = R.Checker()
    done = set()
    for case in MR.limit_cases(True):
        check_spatial(lib, ops, ck, case)
        done.add(case)
    for case in MR.limit_cases(False):
        if case not in done:
            check_spatial(lib, ops, ck, case, backward=MR.accepted(case.h, case.w, True))
    finish(ck)


def test_spatial_refusals_enqueue_nothing(lib, ops):
    """Grids past the LDS tile are refused with the documented message and leave every output as it was; 14 × 15 runs forward and is refused backward."""
    ck = R.Checker()
    for bwd in (False, True):
        for h, w in MR.refused_grids(bwd) + ([(14, 15)] if bwd else []):
            for dt in DT:
                case = MR.Case(dt, "hybrid", "A", 2, h, w, 0.0, None)
                s = Spatial(lib, ops, case)
                ctx = s.ctx + (" backward" if bwd else " forward")
                want = MR.REFUSAL.format(h=h, w=w)
                if bwd:
                    rc, dto, grads, ws = s.bwd()
                    outs = [dto, ws]
                else:
                    rc, d = s.fwd()
                    outs, grads = [d], {}
                torch.cuda.synchronize()
                if rc == 0 or want not in last_error():
                    ck.fail("refusal", ctx, f"rc={rc}, message {last_error()!r}, expected {want!r}")
                for o in outs:
                    if not bool(torch.isnan(o.buf).all()):
                        ck.fail("refusal", ctx, "an output was written")
                for i, (k, g) in enumerate(grads.items()):
                    ck.exact("refusal leaves the gradients", g.t, prefill(g.t.numel(), i), ctx)
                guards(ck, "guards", ctx, *grads.values())
    for dt in DT:       # accepted forward although the backward refuses it
        check_spatial(lib, ops, ck, MR.Case(dt, "hybrid", "A", 2, 14, 15, 0.1, MR.DROP_SEEDS[0]), backward=False)
    finish(ck)


def test_spatial_image_sum_reduction(lib, ops):
    """Image counts on both sides of the reduce kernel's 16 phases and its 4× unroll; two identical launches return the same bits."""
    ck = R.Checker()
    for case in MR.IMAGE_SUM_CASES:
        check_spatial(lib, ops, ck, case, twice=True, wrapper=case.B in (17, 113))
    finish(ck)


def test_spatial_atomic_path_without_workspace(lib, ops):
    """ws = NULL, the C entry alone: every image adds its share with float atomics; bounds only."""
    ck = R.Checker()
    for case in MR.ATOMIC_CASES:
        check_spatial(lib, ops, ck, case, workspace=False, wrapper=False)
    finish(ck)


def test_spatial_per_pixel_kernel_bf16_at_widths_14_and_4():
    """UIA_MONA_FAST=0 is read once per process, so the cases run in one fresh child: the fast kernel's cases on the per-pixel kernel, judged
    without the matrix-core term."""
    env = dict(os.environ, UIA_MONA_FAST="0")
    r = subprocess.run([sys.executable, DRIVER], env=env, capture_output=True, text=True, timeout=240)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    assert "0 failing comparisons" in r.stdout


# ------------------------------------------------------------------------------------------ pre-norm
def pre_dev(x, du, dy, nw, nb, gamma, gammax):
    return [up(v) for v in (x, du, dy, nw, nb, gamma, gammax)]


def pre_shapes():
    for D in MR.PRE_D:
        for M in MR.PRE_M:
            yield M, D, 0.0
    for M, D in MR.PRE_LONG:
        yield M, D, 0.0
    yield 37, 256, 1000.0            # rows of mean 1000 and deviation 1
    yield 6, 768, 1000.0


def test_pre_forward(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, (M, D, mean) in enumerate(pre_shapes()):
            ctx = f"{dt} M={M} D={D} mean={mean}"
            x, du, dy, nw, nb, gamma, gammax = MR.pre_operands(M, D, dt, i, mean)
            xd, _, _, nwd, nbd, gd, gxd = pre_dev(x, du, dy, nw, nb, gamma, gammax)
            ref = MR.pre_fwd(x, nw, nb, gamma, gammax)["u"]
            u = Out((M, D), dt)
            if not call(ck, ctx, "uia_mona_pre_fwd", lib.uia_mona_pre_fwd(ops._stream(), ops._code(dt), M, D, p(xd), p(nwd), p(nbd), p(gd), p(gxd), MR.EPS, p(u))):
                continue
            ck.check(bar("pre fwd u" + (" (mean 1000)" if mean else ""), dt), u.t, ref.ref, MR.bound(ref, MR.C_U, dt), ctx)
            guards(ck, "guards", ctx, u)
            u2 = torch.full((M, D), float("nan"), dtype=dt, device=dev())
            ops.mona_pre_fwd(xd, nwd, nbd, gd, gxd, u2, MR.EPS)
            ck.exact("wrapper u", u2, u.t, ctx)
    finish(ck)


def test_pre_refusals_enqueue_nothing(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for D in MR.PRE_D_REFUSED:
            M = 3
            ctx = f"{dt} M={M} D={D}"
            x, du, dy, nw, nb, gamma, gammax = MR.pre_operands(M, D, dt, D)
            xd, dud, dyd, nwd, nbd, gd, gxd = pre_dev(x, du, dy, nw, nb, gamma, gammax)
            u, dx = Out((M, D), dt), Out((M, D), F32)
            gg = [Out((D,), F32, init=prefill(D, k)) for k in range(4)]
            ws = Out((4096,), F32)
            rc1 = lib.uia_mona_pre_fwd(ops._stream(), ops._code(dt), M, D, p(xd), p(nwd), p(nbd), p(gd), p(gxd), MR.EPS, p(u))
            msg1 = last_error()
            rc2 = lib.uia_mona_pre_bwd(ops._stream(), ops._code(dt), M, D, p(dud), p(xd), p(dyd), p(nwd), p(nbd), p(gd), p(gxd), MR.EPS, p(dx), None, *(p(g) for g in gg), p(ws), 0)
            msg2 = last_error()
            torch.cuda.synchronize()
            if rc1 == 0 or rc2 == 0 or "unsupported shape" not in msg1 or "unsupported shape" not in msg2:
                ck.fail("refusal", ctx, f"rc={rc1}, {rc2}: {msg1!r}, {msg2!r}")
            if not all(bool(torch.isnan(o.buf).all()) for o in (u, dx, ws)):
                ck.fail("refusal", ctx, "an output was written")
            for k, g in enumerate(gg):
                ck.exact("refusal leaves the gradients", g.t, prefill(D, k), ctx)
    finish(ck)


GRADS = ("g_gamma", "g_gammax", "g_nw", "g_nb")


def pre_bwd_case(lib, ops, ck, ctx, dt, M, D, ops_cpu, ops_dev, refs, mode, kb_rows=0, tag=""):
    """One guarded uia_mona_pre_bwd launch in `mode` ("both", "dx32", "dxT", "none") and the same through the wrapper: returns the row-major dxT."""
    xd, dud, dyd, nwd, nbd, gd, gxd = ops_dev
    want32, wantT = mode in ("both", "dx32"), mode in ("both", "dxT")
    g = 64 // torch.empty(0, dtype=dt).element_size()
    dx32 = Out((M, D), F32) if want32 else None
    dxT = (Out((D // g, kb_rows, g), dt) if kb_rows else Out((M, D), dt)) if wantT else None
    gg = [Out((D,), F32, init=prefill(D, k)) for k in range(4)]
    ws = Out((lib.uia_mona_pre_bwd_workspace_bytes(M, D) // 4,), F32)
    dy_ = None if mode == "none" else dyd
    if not call(ck, ctx, "uia_mona_pre_bwd", lib.uia_mona_pre_bwd(ops._stream(), ops._code(dt), M, D, p(dud), p(xd), p(dy_), p(nwd), p(nbd), p(gd), p(gxd), MR.EPS,
                                                                  p(dx32), p(dxT), *(p(o) for o in gg), p(ws), kb_rows)):
        return None
    name = "pre bwd" + tag
    if want32:
        ck.check(name + " dx32", dx32.t, refs["dx"].ref, MR.bound(refs["dx"], MR.C_DX, F32), ctx)
    if wantT and not kb_rows:
        ck.check(bar(name + " dxT", dt), dxT.t, refs["dx"].ref, MR.bound(refs["dx"], MR.C_DX, dt), ctx)
    for k, o in zip(GRADS, gg):
        pre = prefill(D, GRADS.index(k))
        ck.check(f"{name} {k}", o.t, refs[k].ref + pre.to(torch.float64), MR.bound(refs[k], MR.pre_count(k, M), F32, prefill=pre), ctx)
    guards(ck, "guards", ctx, ws, *gg, *[o for o in (dx32, dxT) if o is not None])
    # the wrapper
    w32 = torch.full((M, D), float("nan"), dtype=F32, device=dev()) if want32 else None
    if wantT and kb_rows:
        whole = torch.full((D // g, kb_rows, g), float("nan"), dtype=dt, device=dev())
        wT = ops.KBlocked(whole).row_range(0, M)
    else:
        whole = wT = torch.full((M, D), float("nan"), dtype=dt, device=dev()) if wantT else None
    g2 = [up(prefill(D, k)) for k in range(4)]
    ops.mona_pre_bwd(dud, xd, dy_, nwd, nbd, gd, gxd, w32, wT, *g2, eps=MR.EPS)
    if want32:
        ck.exact("wrapper dx32", w32, dx32.t, ctx)
    if wantT:
        ck.exact("wrapper dxT", whole, dxT.t, ctx)
    return dxT


def test_pre_backward(lib, ops):
    """Every output combination at every width and small row count; the K-blocked copy is the row-major copy permuted, bit for bit, and leaves its
    padding rows alone."""
    ck = R.Checker()
    for dt in DT:
        g = 64 // torch.empty(0, dtype=dt).element_size()
        for i, (M, D, mean) in enumerate(pre_shapes()):
            ctx = f"{dt} M={M} D={D} NV={MR.pre_nv(D)} mean={mean}"
            cpu = MR.pre_operands(M, D, dt, i, mean)
            x, du, dy, nw, nb, gamma, gammax = cpu
            devs = pre_dev(*cpu)
            refs = MR.pre_bwd(du, x, dy, nw, nb, gamma, gammax)
            tag = " (mean 1000)" if mean else ""
            long = M > 1000
            rowT = pre_bwd_case(lib, ops, ck, ctx + " both", dt, M, D, cpu, devs, refs, "both", tag=tag)
            if not long:
                for mode in ("dx32", "dxT", "none"):
                    pre_bwd_case(lib, ops, ck, f"{ctx} {mode}", dt, M, D, cpu, devs, refs, mode, tag=tag)
            if D % g == 0 and rowT is not None:
                for kb_rows in ((M + 3,) if long else (M, M + 3)):
                    kb = pre_bwd_case(lib, ops, ck, f"{ctx} dxT_kb_rows={kb_rows}", dt, M, D, cpu, devs, refs, "both" if kb_rows == M else "dxT", kb_rows=kb_rows, tag=tag)
                    if kb is not None:
                        ck.exact("K-blocked dxT = row-major dxT permuted", kb.t, MR.kb_layout(rowT.t.cpu(), kb_rows, dt), f"{ctx} dxT_kb_rows={kb_rows}")
    finish(ck)
