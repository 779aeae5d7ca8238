"""-m gpu: what the LayerNorm kernels of csrc/layernorm.hip (forward, backward, its three-byte and periodic variants), uia_ln_mean_rows of
csrc/dino_pool.hip, uia_rows3_to_f32 and the three-byte codec of csrc/uia_common.h must compute, element by element against the float64 restatements of
tests/layernorm_reference.py on the operands the kernel sees, at the case tables of that module (both sides of the NV switch, partly used float4
groups, row counts that are no multiple of a workgroup's four, strided rows, K-blocked planes with more rows than M, periods that do not divide M,
pool slices below, at and above 32 rows).

Every output is a view inside a guarded buffer (tests/guarded_out.py; int8 planes in Out8 below), strided outputs keep their padding columns, and
strided inputs carry NaN in theirs, so a read or a write beside a row shows.  An output that a case does not ask for is a null pointer: there is nothing
of it to touch, and the guards of the outputs it does ask for are what a stray write would hit.  The calls go to the C entry points; each case also runs through its
uia_hip.ops wrapper, whose bits must equal the C call's.  Each test loops over its cases and fails once with the collected list (bar, case, worst flat
index, error/bound); the bounds are derived in layernorm_reference, none is fitted to what a kernel returns."""
import pytest
import torch

import helpers_reference as R
import layernorm_reference as LR
from guarded_out import PAD, Out, dev, guards

pytestmark = pytest.mark.gpu

F32, BF16, I8 = torch.float32, torch.bfloat16, torch.int8
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from uia_hip import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from uia_hip import _lib
    return _lib.lib()


class Out8:
    """An int8 [rows, cols] output inside a buffer of sentinel bytes with guard bytes on both sides."""
    SENTINEL = 0x5A

    def __init__(self, rows, cols):
        self.n = rows * cols
        self.buf = torch.full((PAD + self.n + PAD,), self.SENTINEL, dtype=I8, device=dev())
        self.t = self.buf[PAD:PAD + self.n].view(rows, cols)

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == self.SENTINEL).all()) and bool((b[PAD + self.n:] == self.SENTINEL).all())


def up(t, dt=None):
    return None if t is None else t.to(dt if dt is not None else t.dtype).to(dev()).contiguous()


def strided(t, ld, dt=None):
    """A CPU [M, D] tensor as the first D columns of a NaN-filled device [M, ld]."""
    if t is None:
        return None
    M, D = t.shape
    dt = dt or t.dtype
    buf = torch.full((M, ld), NAN if dt.is_floating_point else Out8.SENTINEL, dtype=dt, device=dev())
    buf[:, :D] = t.to(dev())
    return buf[:, :D]


def p(t):
    return None if t is None else (t.t if isinstance(t, (Out, Out8)) else t).data_ptr()


def call(ck, ctx, name, rc):
    if rc != 0:
        from uia_hip import _lib
        ck.fail(name, ctx, f"rc={rc}: {_lib.lib().uia_last_error().decode()}")
    return rc == 0


def finish(ck):
    assert ck.ok(), ck.report()
    print(ck.report())


def tag(dt):
    return "bf16" if dt == BF16 else "fp32"


def nan_like(o):
    return None if o is None else torch.full(tuple(o.t.shape), NAN, dtype=o.t.dtype, device=dev())


# ------------------------------------------------------------------------------------------ forward
def test_forward_outputs_and_stats_at_every_width_row_count_and_stride(lib, ops):
    ck = R.Checker()
    for case in LR.fwd_cases():
        ctx, dt, M, D = LR.name_of(case), case.dtype, case.M, case.D
        x, gamma, beta = LR.fwd_inputs(case)
        ref = LR.ln_fwd(x, gamma, beta, case.eps)
        ld = LR.ld_of(case.ld, D)
        xd, gd, bd = strided(x, ld), up(gamma), up(beta)
        yT = Out((M, D), dt) if "yT" in case.outs else None
        y32 = Out((M, D), F32) if "y32" in case.outs else None
        st = Out((M, 2), F32) if "stats" in case.outs else None
        if st is not None:
            rc = lib.uia_layernorm_fwd_stats(ops._stream(), ops._code(dt), M, D, ld, p(xd), p(gd), p(bd), case.eps, p(yT), p(y32), p(st))
        else:
            rc = lib.uia_layernorm_fwd(ops._stream(), ops._code(dt), M, D, ld, p(xd), p(gd), p(bd), case.eps, p(yT), p(y32))
        if not call(ck, ctx, "uia_layernorm_fwd", rc):
            continue
        if yT is not None:
            ck.check(f"fwd yT {tag(dt)}", yT.t, ref["y"].ref, LR.bound(ref["y"], dt), ctx)
        if y32 is not None:
            ck.check("fwd y32", y32.t, ref["y"].ref, LR.bound(ref["y"], F32), ctx)
        if yT is not None and y32 is not None:
            ck.exact(f"fwd yT is the {tag(dt)} copy of y32", yT.t, y32.t.to(dt), ctx)
        if st is not None:
            ck.check("fwd stats mean", st.t[:, 0], ref["mean"].ref, LR.bound(ref["mean"], F32), ctx)
            ck.check("fwd stats rstd", st.t[:, 1], ref["rstd"].ref, LR.bound(ref["rstd"], F32), ctx)
        guards(ck, "guards", ctx, *[o for o in (yT, y32, st) if o is not None])
        w = [nan_like(o) for o in (yT, y32, st)]
        ops.layernorm_fwd(xd, gd, bd, case.eps, y_t=w[0], y32=w[1], rows=M, ldx=ld, stats=w[2])
        for name, a, b in zip(("yT", "y32", "stats"), w, (yT, y32, st)):
            if b is not None:
                ck.exact("wrapper " + name, a, b.t, ctx)
    finish(ck)


# ------------------------------------------------------------------------------------------ backward
def test_backward_with_and_without_a_residual_gradient_on_strided_rows(lib, ops):
    ck = R.Checker()
    for case in LR.bwd_cases():
        ctx, dt, M, D = LR.name_of(case), case.dtype, case.M, case.D
        dy, x, gamma, dres = LR.bwd_inputs(case)
        ref = LR.ln_bwd(dy, x, gamma, case.eps, dres)
        ld = LR.ld_of(case.ld, D)
        xd, gd, rd = strided(x, ld), up(gamma), strided(dres, ld)
        for zero_dy in (False, True):
            dyd = torch.zeros(M, D, dtype=dt, device=dev()) if zero_dy else up(dy, dt)
            dx32 = Out((M, D), F32, ld=ld) if "dx32" in case.outs else None
            dxT = Out((M, D), dt, ld=ld) if "dxT" in case.outs else None
            rc = lib.uia_layernorm_bwd(ops._stream(), ops._code(dt), M, D, ld, p(dyd), p(xd), p(gd), case.eps, p(rd), p(dx32), p(dxT))
            if not call(ck, ctx, "uia_layernorm_bwd", rc):
                continue
            if zero_dy:                                   # dy = 0: dx is the residual gradient itself
                want = dres if dres is not None else torch.zeros(M, D)
                if dx32 is not None:
                    ck.exact("bwd dy = 0: dx32 is dres", dx32.t, want, ctx)
                if dxT is not None:
                    ck.exact("bwd dy = 0: dxT is dres", dxT.t, want.to(dt), ctx)
            else:
                if dx32 is not None:
                    ck.check("bwd dx32", dx32.t, ref.ref, LR.bound(ref, F32), ctx)
                if dxT is not None:
                    ck.check(f"bwd dxT {tag(dt)}", dxT.t, ref.ref, LR.bound(ref, dt), ctx)
                if dx32 is not None and dxT is not None:
                    ck.exact(f"bwd dxT is the {tag(dt)} copy of dx32", dxT.t, dx32.t.to(dt), ctx)
                w32 = None if dx32 is None else torch.full((M, ld), NAN, dtype=F32, device=dev())
                wT = None if dxT is None else torch.full((M, ld), NAN, dtype=dt, device=dev())
                ops.layernorm_bwd(dyd, xd, gd, case.eps, dres=rd, dx32=w32, dx_t=wT, rows=M, ldx=ld)
                if dx32 is not None:
                    ck.exact("wrapper dx32", w32, dx32.buf[PAD:PAD + M * ld].view(M, ld), ctx)
                if dxT is not None:
                    ck.exact("wrapper dxT", wT, dxT.buf[PAD:PAD + M * ld].view(M, ld), ctx)
            guards(ck, "guards", ctx, *[o for o in (dx32, dxT) if o is not None])
    finish(ck)


# ------------------------------------------------------------------------------------------ three-byte operands and results
def plane_operands(ops, case, planes, name, form):
    """(C pointers hi / lo / kb_rows, wrapper operand) of the three-byte operand `name` of a case."""
    if name + "_hi" not in planes:
        return None, None, 0, None
    hi, lo = planes[name + "_hi"], up(planes[name + "_lo"])
    if form == "kb":
        kb = up(LR.kblock(hi, case.M + case.kb_extra))
        return kb, lo, case.M + case.kb_extra, (ops.KBlocked(kb), lo)
    hi = up(hi)
    return hi, lo, 0, (hi, lo)


def check_three_result(ck, bar, ctx, ref, dx32, dxT, dx_lo):
    if dx32 is not None:
        ck.check(bar + " dx32", dx32.t, ref.ref, LR.bound(ref, F32), ctx)
    if dx_lo is not None:
        ck.check(bar + " decoded (dxT, dx_lo)", LR.decode3(dxT.t.cpu(), dx_lo.t.cpu()), ref.ref, LR.bound(ref, LR.THREE), ctx)
        if dx32 is not None:
            hi, lo = LR.encode3(dx32.t.cpu())
            ck.exact(bar + " dxT is the hi plane of dx32", dxT.t, hi, ctx)
            ck.exact(bar + " dx_lo is the low byte of dx32", dx_lo.t, lo, ctx)
    ck.check(bar + " dxT", dxT.t, ref.ref, LR.bound(ref, BF16), ctx)
    guards(ck, "guards", ctx, *[o for o in (dx32, dxT, dx_lo) if o is not None])


def test_three_byte_operands_row_major_and_k_blocked(lib, ops):
    ck = R.Checker()
    for case in LR.three_cases():
        ctx, M, D = LR.name_of(case), case.M, case.D
        dy, x, gamma, dres, planes = LR.three_inputs(case)
        ref = LR.ln_bwd(dy, x, gamma, case.eps, dres)
        dyd, gd = up(dy, BF16), up(gamma)
        x_hi, x_lo, x_kb, x_w = plane_operands(ops, case, planes, "x", case.x)
        r_hi, r_lo, r_kb, r_w = plane_operands(ops, case, planes, "dres", case.dres)
        xd = up(x) if case.x == "f32" else None
        rd = up(dres) if case.dres == "f32" else None
        dx32 = Out((M, D), F32) if "dx32" in case.outs else None
        dxT = Out((M, D), BF16)
        dx_lo = Out8(M, D) if "dx_lo" in case.outs else None
        rc = lib.uia_layernorm_bwd3(ops._stream(), ops._code(BF16), M, D, D, p(dyd), p(xd), p(x_hi), p(x_lo), x_kb, p(gd), case.eps, p(rd), p(r_hi), p(r_lo), r_kb,
                                    p(dx32), p(dxT), p(dx_lo))
        if not call(ck, ctx, "uia_layernorm_bwd3", rc):
            continue
        check_three_result(ck, "three", ctx, ref, dx32, dxT, dx_lo)
        w32, wT = nan_like(dx32), nan_like(dxT)
        wlo = None if dx_lo is None else torch.full((M, D), Out8.SENTINEL, dtype=I8, device=dev())
        ops.layernorm_bwd(dyd, xd if x_w is None else x_w, gd, case.eps, dres=rd if r_w is None else r_w, dx32=w32, dx_t=wT, dx_lo=wlo)
        for name, a, b in (("dx32", w32, dx32), ("dxT", wT, dxT), ("dx_lo", wlo, dx_lo)):
            if b is not None:
                ck.exact("wrapper " + name, a, b.t, ctx)
    finish(ck)


def test_device_codec_on_chosen_bit_patterns(lib, ops):
    """dy = 0 makes the backward a copy of its residual gradient: an fp32 dres holding the sweep's patterns leaves the kernel through three_byte_store4 and must
    equal encode3 bit for bit (clamp, sign of the low byte, subnormals); a three-byte dres enters through three_byte_decode4 and must leave as decode3 in dx32."""
    ck = R.Checker()
    for D in (1024, 260):                     # both instantiations (NV = 4, 3)
        vals = LR.pad_rows(LR.sweep_values(), D, 1.0)
        M = vals.shape[0]
        x, gd = up(LR.rnd(M, D, seed=D)), up(LR.affine(D, 3)[0])
        dyd = torch.zeros(M, D, dtype=BF16, device=dev())
        dxT, dx_lo = Out((M, D), BF16), Out8(M, D)
        ctx = f"encoder D={D} M={M}"
        rd = up(vals)
        rc = lib.uia_layernorm_bwd3(ops._stream(), ops._code(BF16), M, D, D, p(dyd), p(x), None, None, 0, p(gd), 1e-5, p(rd), None, None, 0, None, p(dxT), p(dx_lo))
        if call(ck, ctx, "uia_layernorm_bwd3", rc):
            hi, lo = LR.encode3(vals)
            ck.exact("device encoder hi", dxT.t, hi, ctx)
            ck.exact("device encoder lo", dx_lo.t, lo, ctx)
            guards(ck, "guards", ctx, dxT, dx_lo)
        shi, slo = LR.sweep_planes()
        hi, lo = LR.pad_rows(shi, D, 1.0), LR.pad_rows(slo, D, 0)
        M = hi.shape[0]
        x = up(LR.rnd(M, D, seed=D + 1))
        dyd = torch.zeros(M, D, dtype=BF16, device=dev())
        dx32, dxT = Out((M, D), F32), Out((M, D), BF16)
        ctx = f"decoder D={D} M={M}"
        hid, lod = up(hi), up(lo)
        rc = lib.uia_layernorm_bwd3(ops._stream(), ops._code(BF16), M, D, D, p(dyd), p(x), None, None, 0, p(gd), 1e-5, None, p(hid), p(lod), 0, p(dx32), p(dxT), None)
        if call(ck, ctx, "uia_layernorm_bwd3", rc):
            ck.exact("device decoder", dx32.t, LR.decode3(hi, lo), ctx)
            guards(ck, "guards", ctx, dx32, dxT)
    finish(ck)


def test_rows3_to_f32_row_major_and_k_blocked(lib, ops):
    ck = R.Checker()
    g = torch.Generator().manual_seed(11)
    for D in (4, 260, 768):
        for stride in (1, 5):
            for form in ("rm", "kb") if D % 32 == 0 else ("rm",):
                rows = 3
                total = (rows - 1) * stride + 2
                hs = torch.randint(0, 65536, (total, D), generator=g, dtype=torch.int64)
                hs = torch.where((hs & 0x7F80) == 0x7F80, hs & 0xBFFF, hs)                        # no inf / NaN upper halves
                hi, lo = LR._bf16_of(hs), torch.randint(-128, 128, (total, D), generator=g, dtype=torch.int64).to(I8)
                want = LR.decode3(hi, lo)[::stride][:rows]
                ctx = f"D={D} stride={stride} {form}"
                dst = Out((rows, D), F32)
                lod = strided(lo, D + 4)
                if form == "kb":
                    kb = up(LR.kblock(hi, total + 2))
                    rc = lib.uia_rows3_to_f32(ops._stream(), rows, D, stride, p(kb), D, total + 2, p(lod), D + 4, p(dst))
                    hw = ops.KBlocked(kb)
                else:
                    hw = strided(hi, D + 8)
                    rc = lib.uia_rows3_to_f32(ops._stream(), rows, D, stride, p(hw), D + 8, 0, p(lod), D + 4, p(dst))
                if not call(ck, ctx, "uia_rows3_to_f32", rc):
                    continue
                ck.exact("rows3_to_f32", dst.t, want, ctx)
                guards(ck, "guards", ctx, dst)
                ck.exact("wrapper rows3_to_f32", ops.rows3_to_f32(hw, lod, stride, torch.full((rows, D), NAN, device=dev())), dst.t, ctx)
    finish(ck)


# ------------------------------------------------------------------------------------------ periodic residual gradient
def test_periodic_residual_gradient_at_periods_that_do_not_divide_m(lib, ops):
    ck = R.Checker()
    for case in LR.periodic_cases():
        ctx, M, D, period = LR.name_of(case), case.M, case.D, case.period
        dy, x, gamma, dres_rows, planes = LR.periodic_inputs(case)
        ref = LR.ln_bwd_periodic(dy, x, gamma, case.eps, dres_rows, period)
        dt = F32 if case.form == "f32" else BF16
        dyd, gd = up(dy, dt), up(gamma)
        three_x = case.form == "bf16x3"
        x_hi, x_lo, x_kb, x_w = plane_operands(ops, case, planes, "x", "kb" if three_x and D % 32 == 0 else "rm")
        xd = None if three_x else up(x)
        rows_ = Out(tuple(dres_rows.shape), F32, init=dres_rows)                    # exactly ceil(M / period) rows between NaN guards
        dense = torch.zeros(M, D)
        dense[0::period] = dres_rows
        if dt == F32:
            sets = (("dx32",), ("dxT",), ("dx32", "dxT"))[case.first % 3]
            dx_lo = d_lo = None
        else:
            sets = (("dxT",), ("dx32", "dxT"))[case.first % 2]
            dx_lo, d_lo = Out8(M, D), Out8(M, D)
        dx32, d32 = (Out((M, D), F32), Out((M, D), F32)) if "dx32" in sets else (None, None)
        dxT, dT = (Out((M, D), dt), Out((M, D), dt)) if "dxT" in sets else (None, None)
        rc = lib.uia_layernorm_bwd_periodic(ops._stream(), ops._code(dt), M, D, p(dyd), p(xd), p(x_hi), p(x_lo), x_kb, p(gd), case.eps, p(rows_), period, p(dx32), p(dxT), p(dx_lo))
        if not call(ck, ctx, "uia_layernorm_bwd_periodic", rc):
            continue
        if dt == F32:
            for name, o in (("dx32", dx32), ("dxT", dxT)):
                if o is not None:
                    ck.check("periodic fp32 " + name, o.t, ref.ref, LR.bound(ref, F32), ctx)
            guards(ck, "guards", ctx, *[o for o in (dx32, dxT) if o is not None])
        else:
            check_three_result(ck, "periodic", ctx, ref, dx32, dxT, dx_lo)
        # the dense kernel on the zero-padded residual gradient: the same bits
        dense = up(dense)
        rc = lib.uia_layernorm_bwd3(ops._stream(), ops._code(dt), M, D, D, p(dyd), p(xd), p(x_hi), p(x_lo), x_kb, p(gd), case.eps, p(dense), None, None, 0, p(d32), p(dT), p(d_lo))
        if call(ck, ctx, "uia_layernorm_bwd3", rc):
            for name, a, b in (("dx32", dx32, d32), ("dxT", dxT, dT), ("dx_lo", dx_lo, d_lo)):
                if a is not None:
                    ck.exact("periodic equals dense " + name, a.t, b.t, ctx)
        w32, wT = nan_like(dx32), nan_like(dxT)
        wlo = None if dx_lo is None else torch.full((M, D), Out8.SENTINEL, dtype=I8, device=dev())
        ops.layernorm_bwd_periodic(dyd, xd if x_w is None else x_w, gd, case.eps, rows_.t, period, dx32=w32, dx_t=wT, dx_lo=wlo)
        for name, a, b in (("dx32", w32, dx32), ("dxT", wT, dxT), ("dx_lo", wlo, dx_lo)):
            if b is not None:
                ck.exact("wrapper " + name, a, b.t, ctx)
        if not rows_.intact():
            ck.fail("guards", ctx, "dres_rows' guards were written")
    finish(ck)


# ------------------------------------------------------------------------------------------ LayerNorm + row pool
def test_pool_slices_below_at_and_above_32_rows(lib, ops):
    ck = R.Checker()
    for case in LR.pool_cases():
        ctx, B, L, D, n, row0 = LR.name_of(case), case.B, case.L, case.D, case.n, case.row0
        x, gamma, beta = LR.pool_inputs(case)
        ref = LR.ln_mean_rows(x, gamma, beta, case.eps, row0, n)
        outside = x.clone()                                   # rows outside [row0, row0 + n) hold NaN: reading one shows
        outside[:, :row0] = NAN
        outside[:, row0 + n:] = NAN
        ldx, ldo = D + 4, D + 8
        xd = strided(outside.reshape(B * L, D), ldx)
        gd, bd = up(gamma), up(beta)
        outs = []
        for _ in range(2):
            out, ws = Out((B, D), F32, ld=ldo), Out((B * LR.POOL_SLICES * D,), F32)
            rc = lib.uia_ln_mean_rows(ops._stream(), B, L, row0, n, D, ldx, p(xd), p(gd), p(bd), case.eps, p(ws), p(out), ldo)
            if not call(ck, ctx, "uia_ln_mean_rows", rc):
                break
            guards(ck, "guards", ctx, out, ws)
            outs.append(out)
        if len(outs) != 2:
            continue
        ck.check("pool", outs[0].t, ref.ref, LR.bound(ref, F32), ctx)
        ck.exact("pool: two runs", outs[1].t, outs[0].t, ctx)
        ck.exact("wrapper pool", ops.ln_mean_rows(up(outside), gd, bd, case.eps, row0, n), outs[0].t, ctx)
    finish(ck)
