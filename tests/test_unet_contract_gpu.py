"""-m gpu: what the kernels of csrc/unet_conv.hip, csrc/unet_bn.hip and csrc/unet_resample.hip must compute, element by element against
the float64 restatements of tests/unet_reference.py on the operands the kernel sees, at the shapes where they branch: non-square grids with
H = 1 or W = 1 alone, pixel-tile tails, the MFMA and the direct forms, split outputs, an unaligned source, channel counts past one sweep of
256, the slice cap, a large mean, resizes that grow one axis and shrink the other.

Every output and every scratch buffer is a view inside a NaN-filled buffer with guard elements on both sides (tests/guarded_out.py), so the
calls go to the C entry points; each case also runs through its uia_hip.ops wrapper, whose result must be bit-identical.  Each test loops over
its cases and fails once with the collected list (bar, case, worst flat index, error/bound)."""
import pytest
import torch

import helpers_reference as R
import unet_reference as UR
from guarded_out import Out, dev, guards

pytestmark = pytest.mark.gpu

DT = (torch.bfloat16, torch.float32)
F32 = torch.float32


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


def call(ck, ctx, name, rc):
    if rc != 0:
        from uia_hip import _lib
        ck.fail(name, ctx, f"rc={rc}: {_lib.lib().uia_last_error().decode()}")
    return rc == 0


def finish(ck):
    assert ck.ok(), ck.report()
    print(ck.report())


def bar(name, dt):
    """A bar of a tensor stored in dt, named per dtype: in bf16 the worst element sits at the rounding of the result itself."""
    return name + (" bf16" if dt == torch.bfloat16 else " fp32")


def pairs(ref, mag):
    return list(zip(ref, mag)) if isinstance(ref, tuple) else [(ref, mag)]


# ------------------------------------------------------------------------------------------ 3x3 convolution
def igemm(lib, ops, ck, ctx, dt, mode, grid, x1, x2, w, bias, n, n1, out_shapes):
    """One guarded uia_conv_igemm call and the same call through ops.conv_igemm: the guarded outputs, after the wrapper's were found to hold
    the same bits."""
    B, H, W = grid
    outs = [Out(s, dt) for s in out_shapes]
    C2 = 0 if x2 is None else x2.shape[3]
    if not call(ck, ctx, "uia_conv_igemm", lib.uia_conv_igemm(ops._stream(), ops._code(dt), mode, B, H, W, x1.shape[3], C2, p(x1), p(x2), n, n1, p(w), p(bias),
                                                              p(outs[0]), p(outs[1]) if len(outs) > 1 else None)):
        return None
    got = ops.conv_igemm(mode, x1, x2, w, n, bias=bias, n1=n1)
    for o, g in zip(outs, got if isinstance(got, tuple) else (got,)):
        ck.exact("wrapper", g, o.t, ctx)
    guards(ck, "guards", ctx, *outs)
    return outs


def conv_operands(case, dt, seed):
    B, H, W, C1, C2, N = case
    Cin = C1 + C2
    x1 = UR.rnd(B, H, W, C1, seed=seed).to(dt)
    x2 = UR.rnd(B, H, W, C2, seed=seed + 50).to(dt) if C2 else None
    w = UR.rnd(N, 9 * Cin, seed=seed + 100, scale=(9 * Cin) ** -0.5).to(dt)
    bias = UR.rnd(N, seed=seed + 150)
    dy = UR.rnd(B, H, W, N, seed=seed + 200).to(dt)
    return x1, x2, w, bias, dy


def test_conv3x3_forward_and_data_gradient(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UR.CONV_MFMA + UR.CONV_DIRECT):
            B, H, W, C1, C2, N = case
            Cin = C1 + C2
            x1, x2, w, bias, dy = conv_operands(case, dt, i)
            c = UR.c_conv(9, Cin)
            for b in (bias, None):
                ctx = f"{dt} {case} bias={b is not None}"
                ref, mag = UR.conv3x3(x1, x2, w, b)
                outs = igemm(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(x1), up(x2), up(w), up(b), N, N, [(B, H, W, N)])
                if outs:
                    ck.check(bar("conv3x3 forward", dt), outs[0].t, ref, R.bound(ref, mag, c, dt), ctx)
            # the data gradient: the same kernel on dy with the flipped rows, two outputs split at C1
            ctx = f"{dt} {case} dgrad n1={C1}"
            ref, mag = UR.conv3x3_dgrad(dy, w, n1=C1)
            shapes = [(B, H, W, C1)] + ([(B, H, W, C2)] if C2 else [])
            outs = igemm(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(dy), None, up(UR.conv3_dgrad_rows(w, Cin)), None, Cin, C1, shapes)
            if outs:
                for o, (r, m) in zip(outs, pairs(ref, mag)):
                    ck.check(bar("conv3x3 dgrad", dt), o.t, r, R.bound(r, m, UR.c_conv(9, N), dt), ctx)
    finish(ck)


def test_conv3x3_unaligned_first_source_stays_within_the_bounds(lib, ops):
    """MFMA shapes with x1 one element into its buffer: the launcher then takes the direct kernel (which kernel ran is not observable from
    here); the result must meet the same bounds and the guards."""
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(((1, 7, 3, 64, 32, 96), (1, 13, 11, 32, 0, 64))):
            B, H, W, C1, C2, N = case
            x1, x2, w, bias, _ = conv_operands(case, dt, 30 + i)
            ctx = f"{dt} {case} x1 one element into its buffer"
            buf = torch.zeros(x1.numel() + 8, dtype=dt, device=dev())
            x1d = buf[1:1 + x1.numel()].view(B, H, W, C1)
            x1d.copy_(x1)
            assert x1d.data_ptr() % 16 != 0 and x1d.is_contiguous()
            ref, mag = UR.conv3x3(x1, x2, w, bias)
            outs = igemm(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), x1d, up(x2), up(w), up(bias), N, N, [(B, H, W, N)])
            if outs:
                ck.check(bar("conv3x3 forward", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(9, C1 + C2), dt), ctx)
    finish(ck)


def wgrad(lib, ops, ck, ctx, dt, mode, grid, x1, x2, dy, n, rows, cols):
    """Two guarded uia_conv_wgrad calls (identical bits wanted) and the wrapper's; scratch guarded at exactly splits·R·Cols floats."""
    B, H, W = grid
    C2 = 0 if x2 is None else x2.shape[3]
    S = lib.uia_conv_wgrad_splits(mode, B, H, W, x1.shape[3], C2, n)
    got = []
    for _ in range(2):
        ws = Out((S * rows * cols,), F32) if S > 1 else None
        dw = Out((rows, cols), F32)
        if not call(ck, ctx, "uia_conv_wgrad", lib.uia_conv_wgrad(ops._stream(), ops._code(dt), mode, B, H, W, x1.shape[3], C2, p(x1), p(x2), n, p(dy), p(ws), p(dw))):
            return None, S
        guards(ck, "guards", ctx, dw, *([ws] if ws else []))
        got.append(dw)
    ck.exact("wgrad deterministic", got[1].t, got[0].t, ctx)
    ck.exact("wrapper", ops.conv_wgrad(mode, x1, x2, dy, n), got[0].t, ctx)
    return got[0], S


def test_conv3x3_weight_gradient(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UR.CONV_MFMA + UR.CONV_DIRECT):
            B, H, W, C1, C2, N = case
            x1, x2, _, _, dy = conv_operands(case, dt, i)
            ctx = f"{dt} {case}"
            ref, mag = UR.conv3x3_wgrad(x1, x2, dy)
            dw, S = wgrad(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(x1), up(x2), up(dy), N, N, 9 * (C1 + C2))
            if dw:
                ck.check("conv3x3 wgrad", dw.t, ref, R.bound(ref, mag, UR.c_wgrad(B * H * W, S)), ctx + f" splits={S}")
    finish(ck)


# ------------------------------------------------------------------------------------------ transposed convolution
def test_conv_transpose_forward_backward_weight_gradient(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UR.CONVT):
            B, h, w_, Cin, Cout = case
            x = UR.rnd(B, h, w_, Cin, seed=i).to(dt)
            rows = UR.rnd(4 * Cout, Cin, seed=i + 100, scale=Cin ** -0.5).to(dt)
            bias = UR.rnd(Cout, seed=i + 50)
            dy = UR.rnd(B, 2 * h, 2 * w_, Cout, seed=i + 150).to(dt)
            for b in (bias, None):
                ctx = f"{dt} {case} bias={b is not None}"
                ref, mag = UR.convt_fwd(x, rows, b)
                outs = igemm(lib, ops, ck, ctx, dt, ops.CONVT_FWD, (B, h, w_), up(x), None, up(rows), up(b), 4 * Cout, 4 * Cout, [(B, 2 * h, 2 * w_, Cout)])
                if outs:
                    ck.check(bar("convt forward", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(1, Cin), dt), ctx)
            ctx = f"{dt} {case}"
            wb = rows.T.contiguous()
            ref, mag = UR.convt_bwd(dy, wb)
            outs = igemm(lib, ops, ck, ctx + " backward", dt, ops.CONVT_BWD, (B, h, w_), up(dy), None, up(wb), None, Cin, Cin, [(B, h, w_, Cin)])
            if outs:
                ck.check(bar("convt backward", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(4, Cout), dt), ctx)
            ref, mag = UR.convt_wgrad(x, dy)
            dw, S = wgrad(lib, ops, ck, ctx + " wgrad", dt, ops.CONVT_FWD, (B, h, w_), up(x), None, up(dy), Cout, 4 * Cout, Cin)
            if dw:
                ck.check("convt wgrad", dw.t, ref, R.bound(ref, mag, UR.c_wgrad(B * h * w_, S)), ctx + f" splits={S}")
    finish(ck)


# ------------------------------------------------------------------------------------------ BatchNorm, column sums
def bn_grid():
    i = 0
    for C in UR.BN_C:
        for M in UR.BN_M:
            yield i, M, C
            i += 1
    yield i, UR.BN_CAP[0], UR.BN_CAP[1]


NBT_GUARD = -7


def bn_train_case(lib, ops, ck, ctx, dt, y, gamma, beta, rm, rv, nbt0, mom, relu):
    """One guarded train-mode uia_bn_fwd call, its comparison with the restatement, and the wrapper's bits."""
    M, C = y.shape
    eps = UR.f32(1e-5)
    r = UR.bn_train(y, gamma, beta, rm, rv, nbt0, UR.f32(mom), eps, relu=relu)
    yd, gd, bd = up(y), up(gamma), up(beta)
    c = UR.c_reduce(M, C)

    def buffers():
        return ((Out((C,), F32, init=rm), Out((C,), F32, init=rv)) if rm is not None else (None, None),
                torch.tensor([NBT_GUARD, nbt0, NBT_GUARD], device=dev()) if nbt0 is not None else None)
    (rmo, rvo), nbt = buffers()
    ws = Out((UR.bn_slices(M) * C * 3,), F32)
    mean, invstd, scale, shift, out = Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
    if not call(ck, ctx, "uia_bn_fwd", lib.uia_bn_fwd(ops._stream(), ops._code(dt), 1, M, C, p(yd), p(gd), p(bd), p(rmo), p(rvo), None if nbt is None else nbt[1:].data_ptr(),
                                                      float(mom), eps, p(ws), p(mean), p(invstd), p(scale), p(shift), int(relu), p(out))):
        return
    for k, o in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift)):
        ck.check("bn " + k, o.t, r[k][0], R.bound(r[k][0], r[k][1], c), ctx)
    ck.check(bar("bn out", dt), out.t, r["out"][0], R.bound(r["out"][0], r["out"][1], c, dt), ctx)
    if rmo is not None:
        ck.check("bn running mean", rmo.t, r["run_mean"][0], R.bound(r["run_mean"][0], r["run_mean"][1], c), ctx)
        ck.check("bn running var", rvo.t, r["run_var"][0], R.bound(r["run_var"][0], r["run_var"][1], c), ctx)
    if nbt is not None and nbt.tolist() != [NBT_GUARD, r["nbt"], NBT_GUARD]:
        ck.fail("bn num_batches_tracked", ctx, f"{nbt.tolist()}, expected {r['nbt']} between the guards")
    guards(ck, "guards", ctx, ws, mean, invstd, scale, shift, out, *([rmo, rvo] if rmo is not None else []))
    # the wrapper: the same bits in every output and buffer
    (rm2, rv2), nbt2 = buffers()
    got = ops.bn_fwd(yd.view(1, 1, M, C), gd, bd, rm2.t if rm2 else None, rv2.t if rv2 else None, None if nbt2 is None else nbt2[1], True, mom, eps, relu=relu)
    for g, o in zip(got, (out, mean, invstd, scale, shift)):
        ck.exact("wrapper", g, o.t, ctx)
    if rm2 is not None:
        ck.exact("wrapper", rm2.t, rmo.t, ctx)
        ck.exact("wrapper", rv2.t, rvo.t, ctx)
    if nbt2 is not None:
        ck.exact("wrapper", nbt2, nbt, ctx)


def test_batchnorm_train(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i)
            mom = UR.BN_MOMENTA[i % 3]
            if i % 4 == 3:                          # no running buffers
                rm = rv = None
            nbt0 = None if i % 5 == 4 else i        # no num_batches_tracked
            for relu in (True, False):
                ctx = f"{dt} M={M} C={C} momentum={mom} running={rm is not None} nbt={nbt0} relu={relu}"
                bn_train_case(lib, ops, ck, ctx, dt, y, gamma, beta, rm, rv, nbt0, mom, relu)
    finish(ck)


def test_batchnorm_train_large_mean_keeps_the_variance(lib, ops):
    """fp32 y = ±1000 + N(0, 1): the bound's variance terms are (y − K)², so a kernel that summed y² fails it."""
    ck = R.Checker()
    for M, C in ((1369, 96), UR.BN_CAP):
        for mean in (1000.0, -1000.0):
            g = torch.Generator().manual_seed(int(M + mean))
            y = mean + torch.randn(M, C, generator=g)
            _, gamma, beta, rm, rv = UR.bn_case(M, C, F32, seed=C)
            bn_train_case(lib, ops, ck, f"fp32 M={M} C={C} y = {mean} + N(0, 1)", F32, y, gamma, beta, rm, rv, 0, 0.1, True)
    finish(ck)


def test_batchnorm_eval_leaves_the_buffers(lib, ops):
    ck = R.Checker()
    eps = UR.f32(1e-5)
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i)
            yd, gd, bd = up(y), up(gamma), up(beta)
            for relu in (True, False):
                ctx = f"{dt} M={M} C={C} eval relu={relu}"
                ref, mag = UR.bn_eval(y, gamma, beta, rm, rv, eps, relu=relu)
                rmo, rvo = Out((C,), F32, init=rm), Out((C,), F32, init=rv)
                nbt = torch.tensor([NBT_GUARD, 5, NBT_GUARD], device=dev())
                scale, shift, out = Out((C,), F32), Out((C,), F32), Out((M, C), dt)
                if not call(ck, ctx, "uia_bn_fwd", lib.uia_bn_fwd(ops._stream(), ops._code(dt), 0, M, C, p(yd), p(gd), p(bd), p(rmo), p(rvo), nbt[1:].data_ptr(), 0.1, eps,
                                                                  None, None, None, p(scale), p(shift), int(relu), p(out))):
                    continue
                ck.check(bar("bn eval", dt), out.t, ref, R.bound(ref, mag, UR.C_BN_EVAL, dt), ctx)
                ck.exact("bn eval buffers", rmo.t, rm, ctx)
                ck.exact("bn eval buffers", rvo.t, rv, ctx)
                if nbt.tolist() != [NBT_GUARD, 5, NBT_GUARD]:
                    ck.fail("bn eval buffers", ctx, f"num_batches_tracked {nbt.tolist()}")
                guards(ck, "guards", ctx, rmo, rvo, scale, shift, out)
                got = ops.bn_fwd(yd.view(1, 1, M, C), gd, bd, up(rm), up(rv), nbt[1], False, 0.1, eps, relu=relu)
                ck.exact("wrapper", got[0], out.t, ctx)
                if got[1] is not None or got[2] is not None:
                    ck.fail("wrapper", ctx, "eval mode returned batch statistics")
    finish(ck)


def test_batchnorm_relu_backward(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            ctx = f"{dt} M={M} C={C}"
            y, dout, scale, shift, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=i)
            r = UR.bn_relu_bwd(y, dout, scale, shift, mean, invstd, gamma)
            assert int((r["z"] <= r["band"]).sum()) == 0, ctx
            dev_in = [up(t) for t in (y, dout, scale, shift, mean, invstd, gamma)]
            ws, dgamma, dbeta, dy = Out((UR.bn_slices(M) * C * 3,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
            if not call(ck, ctx, "uia_bn_relu_bwd", lib.uia_bn_relu_bwd(ops._stream(), ops._code(dt), M, C, *(p(t) for t in dev_in), p(ws), p(dgamma), p(dbeta), p(dy))):
                continue
            c = UR.c_reduce(M, C)
            ck.check(bar("bn bwd dy", dt), dy.t, r["dy"][0], R.bound(r["dy"][0], r["dy"][1], c, dt), ctx)
            ck.check("bn bwd dgamma", dgamma.t, r["dgamma"][0], R.bound(r["dgamma"][0], r["dgamma"][1], c), ctx)
            ck.check("bn bwd dbeta", dbeta.t, r["dbeta"][0], R.bound(r["dbeta"][0], r["dbeta"][1], c), ctx)
            guards(ck, "guards", ctx, ws, dgamma, dbeta, dy)
            got = ops.bn_relu_bwd(dev_in[0].view(1, 1, M, C), dev_in[1].view(1, 1, M, C), *dev_in[2:])
            for g, o in zip(got, (dy, dgamma, dbeta)):
                ck.exact("wrapper", g, o.t, ctx)
    finish(ck)


def test_colsum_ordered(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            ctx = f"{dt} M={M} C={C}"
            y = UR.bn_case(M, C, dt, seed=i, mean=0.25)[0]
            yd = up(y)
            ref, mag = UR.colsum(y)
            got = []
            for _ in range(2):
                ws, out = Out((UR.bn_slices(M) * C * 3,), F32), Out((C,), F32)
                if call(ck, ctx, "uia_colsum_ordered", lib.uia_colsum_ordered(ops._stream(), ops._code(dt), M, C, p(yd), p(ws), p(out))):
                    guards(ck, "guards", ctx, ws, out)
                    got.append(out)
            if len(got) == 2:
                ck.check("colsum", got[0].t, ref, R.bound(ref, mag, UR.c_reduce(M, C)), ctx)
                ck.exact("colsum deterministic", got[1].t, got[0].t, ctx)
                ck.exact("wrapper", ops.colsum_ordered(yd), got[0].t, ctx)
    finish(ck)


# ------------------------------------------------------------------------------------------ resampling
def test_upsample_align_corners_forward_backward(lib, ops):
    ck = R.Checker()
    B = 2
    for dt in DT:
        for f in UR.UPS_F:
            for H, W in UR.UPS_HW:
                for C in UR.UPS_C:
                    ctx = f"{dt} f={f} {H}x{W} C={C}"
                    x = UR.rnd(B, H, W, C, seed=f + 10 * H + W).to(dt)
                    dy = UR.rnd(B, H * f, W * f, C, seed=f + H + 10 * W).to(dt)
                    for backward, src, shape, c in ((0, x, (B, H * f, W * f, C), UR.C_UPSAMPLE_AC), (1, dy, (B, H, W, C), UR.c_upsample_ac_bwd(f))):
                        name = bar("upsample_ac backward" if backward else "upsample_ac forward", dt)
                        ref, mag = UR.upsample_ac(src, f, backward=bool(backward))
                        sd, out = up(src), Out(shape, dt)
                        if not call(ck, ctx, "uia_upsample_ac", lib.uia_upsample_ac(ops._stream(), ops._code(dt), backward, B, H, W, C, f, p(sd), p(out))):
                            continue
                        ck.check(name, out.t, ref, R.bound(ref, mag, c, dt), ctx)
                        guards(ck, "guards", ctx, out)
                        ck.exact("wrapper", ops.upsample_ac(sd, f, backward=bool(backward)), out.t, ctx)
    finish(ck)


def test_resize_antialiased_forward_backward(lib, ops):
    ck = R.Checker()
    B = 2
    for dt in DT:
        for (Hi, Wi), (Ho, Wo) in UR.AA_SIZES:
            for C in UR.AA_C:
                ctx = f"{dt} {Hi}x{Wi}->{Ho}x{Wo} C={C}"
                x = UR.rnd(B, Hi, Wi, C, seed=Hi + 10 * Wo + C).to(dt)
                dy = UR.rnd(B, C, Ho, Wo, seed=Wi + 10 * Ho + C)
                xd, dyd = up(x), up(dy)
                ref, mag = UR.resize_aa(x, (Ho, Wo))
                tmp, out = Out((B * C * Hi * Wo,), F32), Out((B, C, Ho, Wo), F32)
                if call(ck, ctx, "uia_resize_aa", lib.uia_resize_aa(ops._stream(), ops._code(dt), 0, B, C, Hi, Wi, Ho, Wo, p(xd), p(tmp), p(out), None, None)):
                    ck.check("resize_aa forward", out.t, ref, R.bound(ref, mag, UR.C_RESIZE_AA), ctx)
                    if (Hi, Wi) == (Ho, Wo):        # every weight is 0 or 1: the input's values, bit for bit
                        ck.exact("resize_aa identity", out.t, x.float().permute(0, 3, 1, 2).contiguous(), ctx)
                    guards(ck, "guards", ctx, tmp, out)
                    ck.exact("wrapper", ops.resize_aa(xd, (Ho, Wo)), out.t, ctx)
                ref, mag = UR.resize_aa_bwd(dy, (Hi, Wi))
                tmp, dx = Out((B * C * Hi * Wo,), F32), Out((B, Hi, Wi, C), dt)
                if call(ck, ctx, "uia_resize_aa", lib.uia_resize_aa(ops._stream(), ops._code(dt), 1, B, C, Hi, Wi, Ho, Wo, None, p(tmp), None, p(dyd), p(dx))):
                    ck.check(bar("resize_aa backward", dt), dx.t, ref, R.bound(ref, mag, UR.C_RESIZE_AA_BWD, dt), ctx + " backward")
                    guards(ck, "guards", ctx + " backward", tmp, dx)
                    ck.exact("wrapper", ops.resize_aa_bwd(dyd, (Hi, Wi), dt), dx.t, ctx + " backward")
    finish(ck)
