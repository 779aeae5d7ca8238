"""-m gpu: what the kernels the UNet baseline added must compute, element by element against the float64 restatements of
tests/unet_baseline_reference.py (and tests/unet_reference.py for the convolutions) on the operands the kernel sees, in both dtypes:
max-pool forward / backward (csrc/unet_pool.hip, exact), the convolutions at channel counts that are multiples of 8 but not of 32 and the 1x1
mode (csrc/unet_conv.hip: the generalised MFMA instantiation, K steps zero-filled past K), BatchNorm + LeakyReLU + dropout (csrc/unet_bn.hip).

As in tests/test_unet_contract_gpu.py every output and scratch buffer is a view inside a NaN-filled buffer with guard elements on both sides,
the calls go to the C entry points, and each case also runs through its uia_hip.ops wrapper, whose result must be bit-identical."""
import pytest
import torch

import helpers_reference as R
import unet_baseline_reference as UB
import unet_reference as UR
from guarded_out import Out, dev, guards

pytestmark = pytest.mark.gpu

DT = (torch.bfloat16, torch.float32)
F32 = torch.float32
SLOPE = 0.01


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
    return name + (" bf16" if dt == torch.bfloat16 else " fp32")


def pairs(ref, mag):
    return list(zip(ref, mag)) if isinstance(ref, tuple) else [(ref, mag)]


# ------------------------------------------------------------------------------------------ max-pool
def pool_case(lib, ops, ck, ctx, dt, x, xd):
    """x: the CPU operand, xd: the same values on the device (possibly an unaligned view)."""
    B, H, W, C = x.shape
    ref, _ = UB.maxpool2(x)
    y = Out((B, H // 2, W // 2, C), dt)
    if not call(ck, ctx, "uia_maxpool2_fwd", lib.uia_maxpool2_fwd(ops._stream(), ops._code(dt), B, H, W, C, xd.data_ptr(), p(y))):
        return
    ck.exact("maxpool forward", y.t, ref.to(dt), ctx)
    ck.exact("wrapper", ops.maxpool2(xd), y.t, ctx)
    dy = UR.rnd(B, H // 2, W // 2, C, seed=B + H + W + C).to(dt)
    dyd = up(dy)
    dx = Out((B, H, W, C), dt)
    if not call(ck, ctx, "uia_maxpool2_bwd", lib.uia_maxpool2_bwd(ops._stream(), ops._code(dt), B, H, W, C, xd.data_ptr(), p(dyd), p(dx))):
        return
    if bool(torch.isnan(dx.t).any()):
        ck.fail("maxpool backward", ctx, "dx holds NaN: an element was not written")
    ck.exact("maxpool backward", dx.t, UB.maxpool2_bwd(x, dy).to(dt), ctx)
    ck.exact("wrapper", ops.maxpool2_bwd(xd, dyd), dx.t, ctx)
    guards(ck, "guards", ctx, y, dx)


def test_maxpool_forward_backward_exact(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, shape in enumerate(UB.POOL):
            for j, kind in enumerate(UB.POOL_DATA):
                x = UB.pool_data(kind, shape, dt, 10 * i + j)
                pool_case(lib, ops, ck, f"{dt} {shape} {kind}", dt, x, up(x))
        # an input one element into its buffer: the scalar form
        for shape in ((2, 4, 6, 24), (1, 5, 7, 8)):
            x = UB.pool_data("random", shape, dt, 77)
            buf = torch.zeros(x.numel() + 8, dtype=dt, device=dev())
            xd = buf[1:1 + x.numel()].view(shape)
            xd.copy_(x)
            assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
            pool_case(lib, ops, ck, f"{dt} {shape} x one element into its buffer", dt, x, xd)
    finish(ck)


def test_maxpool_refuses_a_grid_under_two(lib, ops):
    from uia_hip._lib import UiaError
    for dt in DT:
        for shape in ((1, 1, 4, 8), (1, 4, 1, 8)):
            x = torch.zeros(shape, dtype=dt, device=dev())
            y = Out((1, max(shape[1] // 2, 1), max(shape[2] // 2, 1), 8), dt)
            assert lib.uia_maxpool2_fwd(ops._stream(), ops._code(dt), *shape, x.data_ptr(), p(y)) != 0
            assert b"2x2" in lib.uia_last_error()
            dx = Out(shape, dt)
            assert lib.uia_maxpool2_bwd(ops._stream(), ops._code(dt), *shape, x.data_ptr(), p(y), p(dx)) != 0
            assert y.intact() and dx.intact() and bool(torch.isnan(dx.t).all())
            with pytest.raises(UiaError, match="2x2"):
                ops.maxpool2(x)
            with pytest.raises(UiaError, match="2x2"):
                ops.maxpool2_bwd(x, y.t)


# ------------------------------------------------------------------------------------------ convolutions
def igemm(lib, ops, ck, ctx, dt, mode, grid, x1, x2, w, bias, n, n1, out_shapes):
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


def wgrad(lib, ops, ck, ctx, dt, mode, grid, x1, x2, dy, n, rows, cols):
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


def conv_operands(case, dt, seed, taps=9):
    B, H, W, C1, C2, N = case
    Cin = C1 + C2
    x1 = UR.rnd(B, H, W, C1, seed=seed).to(dt)
    x2 = UR.rnd(B, H, W, C2, seed=seed + 50).to(dt) if C2 else None
    w = UR.rnd(N, taps * Cin, seed=seed + 100, scale=(taps * Cin) ** -0.5).to(dt)
    bias = UR.rnd(N, seed=seed + 150)
    dy = UR.rnd(B, H, W, N, seed=seed + 200).to(dt)
    return x1, x2, w, bias, dy


def test_conv3x3_at_channel_multiples_of_eight(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UB.CONV3_CASES):
            B, H, W, C1, C2, N = case
            Cin = C1 + C2
            assert ops.conv_igemm_form(ops.CONV3, C1, C2, N) == 1 and (C1 % 32 or C2 % 32)
            x1, x2, w, bias, dy = conv_operands(case, dt, 300 + i)
            for b in (bias, None):
                ctx = f"{dt} {case} bias={b is not None}"
                ref, mag = UR.conv3x3(x1, x2, w, b)
                outs = igemm(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(x1), up(x2), up(w), up(b), N, N, [(B, H, W, N)])
                if outs:
                    ck.check(bar("conv3x3 forward", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(9, Cin), dt), ctx)
            ctx = f"{dt} {case} dgrad n1={C1}"
            ref, mag = UR.conv3x3_dgrad(dy, w, n1=C1)
            shapes = [(B, H, W, C1)] + ([(B, H, W, C2)] if C2 else [])
            outs = igemm(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(dy), None, up(UR.conv3_dgrad_rows(w, Cin)), None, Cin, C1, shapes)
            if outs:
                for o, (r, m) in zip(outs, pairs(ref, mag)):
                    ck.check(bar("conv3x3 dgrad", dt), o.t, r, R.bound(r, m, UR.c_conv(9, N), dt), ctx)
            ctx = f"{dt} {case} wgrad"
            ref, mag = UR.conv3x3_wgrad(x1, x2, dy)
            dw, S = wgrad(lib, ops, ck, ctx, dt, ops.CONV3, (B, H, W), up(x1), up(x2), up(dy), N, N, 9 * Cin)
            if dw:
                ck.check("conv3x3 wgrad", dw.t, ref, R.bound(ref, mag, UR.c_wgrad(B * H * W, S)), ctx + f" splits={S}")
    finish(ck)


def test_conv3x3_weight_gradient_over_hundreds_of_splits(lib, ops):
    """The narrow shapes split their pixels far more often than the 64 ranges of the wide ones: 128 ranges, and the cap of 512."""
    ck = R.Checker()
    seen = set()
    for dt in DT:
        for i, case in enumerate(UB.WGRAD_SPLIT_CASES):
            B, H, W, C1, C2, N = case
            x1, x2, _, _, dy = conv_operands(case, dt, 700 + i)
            ref, mag = UR.conv3x3_wgrad(x1, x2, dy)
            dw, S = wgrad(lib, ops, ck, f"{dt} {case} wgrad", dt, ops.CONV3, (B, H, W), up(x1), up(x2), up(dy), N, N, 9 * (C1 + C2))
            seen.add(S)
            if dw:
                ck.check("conv3x3 wgrad", dw.t, ref, R.bound(ref, mag, UR.c_wgrad(B * H * W, S)), f"{dt} {case} splits={S}")
    finish(ck)
    assert min(seen) >= 100 and max(seen) == 512, seen


def test_conv1x1_forward_data_and_weight_gradient(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UB.CONV1_CASES):
            B, H, W, C1, _, N = case
            x, _, w, bias, dy = conv_operands(case, dt, 400 + i, taps=1)
            for b in (bias, None):
                ctx = f"{dt} {case} 1x1 bias={b is not None}"
                ref, mag = UB.conv1x1(x, w, b)
                outs = igemm(lib, ops, ck, ctx, dt, ops.CONV1, (B, H, W), up(x), None, up(w), up(b), N, N, [(B, H, W, N)])
                if outs:
                    ck.check(bar("conv1x1 forward", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(1, C1), dt), ctx)
            ctx = f"{dt} {case} 1x1 dgrad"
            wt = w.T.contiguous()
            ref, mag = UB.conv1x1(dy, wt)
            outs = igemm(lib, ops, ck, ctx, dt, ops.CONV1, (B, H, W), up(dy), None, up(wt), None, C1, C1, [(B, H, W, C1)])
            if outs:
                ck.check(bar("conv1x1 dgrad", dt), outs[0].t, ref, R.bound(ref, mag, UR.c_conv(1, N), dt), ctx)
            ctx = f"{dt} {case} 1x1 wgrad"
            ref, mag = UB.conv1x1_wgrad(x, dy)
            dw, S = wgrad(lib, ops, ck, ctx, dt, ops.CONV1, (B, H, W), up(x), None, up(dy), N, N, C1)
            if dw:
                ck.check("conv1x1 wgrad", dw.t, ref, R.bound(ref, mag, UR.c_wgrad(B * H * W, S)), ctx + f" splits={S}")
    finish(ck)


def test_conv1x1_takes_one_source_and_one_output(lib, ops):
    x = torch.zeros(1, 2, 2, 8, dtype=F32, device=dev())
    w = torch.zeros(8, 16, dtype=F32, device=dev())
    y = Out((1, 2, 2, 8), F32)
    assert lib.uia_conv_igemm(ops._stream(), ops._code(F32), ops.CONV1, 1, 2, 2, 8, 8, x.data_ptr(), x.data_ptr(), 8, 8, w.data_ptr(), None, p(y), None) != 0
    assert lib.uia_conv_igemm(ops._stream(), ops._code(F32), ops.CONV1, 1, 2, 2, 8, 0, x.data_ptr(), None, 8, 4, w.data_ptr(), None, p(y), p(y)) != 0
    assert y.intact() and bool(torch.isnan(y.t).all())


def test_conv_transpose_at_channel_multiples_of_eight(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, case in enumerate(UB.CONVT_CASES):
            B, h, w_, Cin, Cout = case
            x = UR.rnd(B, h, w_, Cin, seed=500 + i).to(dt)
            rows = UR.rnd(4 * Cout, Cin, seed=600 + i, scale=Cin ** -0.5).to(dt)
            bias = UR.rnd(Cout, seed=550 + i)
            dy = UR.rnd(B, 2 * h, 2 * w_, Cout, seed=650 + i).to(dt)
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


# ------------------------------------------------------------------------------------------ BatchNorm + LeakyReLU + dropout
def bn_grid():
    i = 0
    for C in UR.BN_C:
        for M in UR.BN_M:
            yield i, M, C
            i += 1


def test_bn_act_train_forward(lib, ops):
    ck = R.Checker()
    eps, mom = UR.f32(1e-5), 0.1
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i, mean=0.3)
            yd, gd, bd = up(y), up(gamma), up(beta)
            c = UR.c_reduce(M, C) + UB.C_ACT
            for pi, pd in enumerate(UB.DROP_P):
                ctx = f"{dt} M={M} C={C} p={pd}"
                keep = UB.keep_rows(M, C, pd, 1000 + 3 * i + pi)
                kd = up(keep)
                r = UB.bn_act_train(y, gamma, beta, rm, rv, 0, UR.f32(mom), eps, SLOPE, pd, keep)
                rmo, rvo = Out((C,), F32, init=rm), Out((C,), F32, init=rv)
                nbt = torch.zeros(1, dtype=torch.int64, device=dev())
                ws = Out((UR.bn_slices(M) * C * 3,), F32)
                mean, invstd, scale, shift, out = Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
                if not call(ck, ctx, "uia_bn_act_fwd", lib.uia_bn_act_fwd(ops._stream(), ops._code(dt), 1, M, C, p(yd), p(gd), p(bd), p(rmo), p(rvo), nbt.data_ptr(), mom, eps,
                                                                          p(ws), p(mean), p(invstd), p(scale), p(shift), SLOPE, p(out), pd, 0, p(kd))):
                    continue
                for k, o in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift), ("run_mean", rmo), ("run_var", rvo)):
                    ck.check("bn_act " + k, o.t, r[k][0], R.bound(r[k][0], r[k][1], c), ctx)
                ck.check(bar("bn_act out", dt), out.t, r["out"][0], R.bound(r["out"][0], r["out"][1], c, dt), ctx)
                if int(nbt) != 1:
                    ck.fail("bn_act num_batches_tracked", ctx, f"{int(nbt)}")
                guards(ck, "guards", ctx, ws, mean, invstd, scale, shift, out, rmo, rvo)
                rm2, rv2, nbt2 = up(rm), up(rv), torch.zeros((), dtype=torch.int64, device=dev())
                got = ops.bn_act_fwd(yd.view(1, 1, M, C), gd, bd, rm2, rv2, nbt2, True, mom, eps, SLOPE, pd, 0, kd.view(1, 1, M, C))
                for g, o in zip(got, (out, mean, invstd, scale, shift)):
                    ck.exact("wrapper", g, o.t, ctx)
                ck.exact("wrapper", rm2, rmo.t, ctx)
                ck.exact("wrapper", rv2, rvo.t, ctx)
    finish(ck)


def test_bn_act_eval_has_no_dropout_and_leaves_the_buffers(lib, ops):
    ck = R.Checker()
    eps = UR.f32(1e-5)
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i, mean=0.3)
            yd, gd, bd = up(y), up(gamma), up(beta)
            ctx = f"{dt} M={M} C={C} eval"
            ref, mag = UB.bn_act_eval(y, gamma, beta, rm, rv, eps, SLOPE)
            rmo, rvo = Out((C,), F32, init=rm), Out((C,), F32, init=rv)
            kd = up(UB.keep_rows(M, C, 0.5, i))
            scale, shift, out = Out((C,), F32), Out((C,), F32), Out((M, C), dt)
            if not call(ck, ctx, "uia_bn_act_fwd", lib.uia_bn_act_fwd(ops._stream(), ops._code(dt), 0, M, C, p(yd), p(gd), p(bd), p(rmo), p(rvo), None, 0.1, eps,
                                                                      None, None, None, p(scale), p(shift), SLOPE, p(out), 0.5, 0, p(kd))):
                continue
            ck.check(bar("bn_act eval", dt), out.t, ref, R.bound(ref, mag, UR.C_BN_EVAL + UB.C_ACT, dt), ctx)
            ck.exact("bn_act eval buffers", rmo.t, rm, ctx)
            ck.exact("bn_act eval buffers", rvo.t, rv, ctx)
            guards(ck, "guards", ctx, rmo, rvo, scale, shift, out)
            got = ops.bn_act_fwd(yd.view(1, 1, M, C), gd, bd, up(rm), up(rv), None, False, 0.1, eps, SLOPE, 0.5, 0, kd.view(1, 1, M, C))
            ck.exact("wrapper", got[0], out.t, ctx)
    finish(ck)


def test_bn_act_backward(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            y, dout, scale, shift, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=i)
            dev_in = [up(t) for t in (y, dout, scale, shift, mean, invstd, gamma)]
            c = UR.c_reduce(M, C) + UB.C_ACT
            for pi, pd in enumerate(UB.DROP_P):
                ctx = f"{dt} M={M} C={C} p={pd}"
                keep = UB.keep_rows(M, C, pd, 2000 + 3 * i + pi)
                kd = up(keep)
                r = UB.bn_act_bwd(y, dout, scale, shift, mean, invstd, gamma, SLOPE, pd, keep)
                assert int((r["z"] <= r["band"]).sum()) == 0, ctx
                ws, dgamma, dbeta, dy = Out((UR.bn_slices(M) * C * 3,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
                if not call(ck, ctx, "uia_bn_act_bwd", lib.uia_bn_act_bwd(ops._stream(), ops._code(dt), M, C, *(p(t) for t in dev_in), p(ws), p(dgamma), p(dbeta), p(dy),
                                                                          SLOPE, pd, 0, p(kd))):
                    continue
                ck.check(bar("bn_act bwd dy", dt), dy.t, r["dy"][0], R.bound(r["dy"][0], r["dy"][1], c, dt), ctx)
                ck.check("bn_act bwd dgamma", dgamma.t, r["dgamma"][0], R.bound(r["dgamma"][0], r["dgamma"][1], c), ctx)
                ck.check("bn_act bwd dbeta", dbeta.t, r["dbeta"][0], R.bound(r["dbeta"][0], r["dbeta"][1], c), ctx)
                guards(ck, "guards", ctx, ws, dgamma, dbeta, dy)
                got = ops.bn_act_bwd(dev_in[0].view(1, 1, M, C), dev_in[1].view(1, 1, M, C), *dev_in[2:], SLOPE, pd, 0, kd.view(1, 1, M, C))
                for g, o in zip(got, (dy, dgamma, dbeta)):
                    ck.exact("wrapper", g, o.t, ctx)
    finish(ck)


def test_bn_act_backward_at_zero_takes_the_slope(lib, ops):
    """scale = shift = 0 makes z exactly 0 at every element: dz = slope·dout·keep/(1 − p) there, as PyTorch's leaky_relu backward."""
    ck = R.Checker()
    for dt in DT:
        for M, C, pd in ((37, 5, 0.0), (257, 96, 0.5)):
            ctx = f"{dt} M={M} C={C} p={pd} z == 0"
            y, dout, _, _, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=M)
            zero = torch.zeros(C)
            keep = UB.keep_rows(M, C, pd, 3000 + M)
            r = UB.bn_act_bwd(y, dout, zero, zero, mean, invstd, gamma, SLOPE, pd, keep)
            assert float(r["z"].max()) == 0.0 and float(r["dbeta"][0].abs().max()) > 0
            dev_in = [up(t) for t in (y, dout, zero, zero, mean, invstd, gamma)]
            ws, dgamma, dbeta, dy = Out((UR.bn_slices(M) * C * 3,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
            if not call(ck, ctx, "uia_bn_act_bwd", lib.uia_bn_act_bwd(ops._stream(), ops._code(dt), M, C, *(p(t) for t in dev_in), p(ws), p(dgamma), p(dbeta), p(dy),
                                                                      SLOPE, pd, 0, p(up(keep)))):
                continue
            c = UR.c_reduce(M, C) + UB.C_ACT
            ck.check(bar("bn_act bwd dy", dt), dy.t, r["dy"][0], R.bound(r["dy"][0], r["dy"][1], c, dt), ctx)
            ck.check("bn_act bwd dgamma", dgamma.t, r["dgamma"][0], R.bound(r["dgamma"][0], r["dgamma"][1], c), ctx)
            ck.check("bn_act bwd dbeta", dbeta.t, r["dbeta"][0], R.bound(r["dbeta"][0], r["dbeta"][1], c), ctx)
            guards(ck, "guards", ctx, ws, dgamma, dbeta, dy)
    finish(ck)


def test_bn_act_eval_with_a_drop_rate_asks_nothing_of_the_element_count(ops):
    y = torch.randn(1, 1, 3, 5, dtype=F32, device=dev())
    g = torch.ones(5, dtype=F32, device=dev())
    a = ops.bn_act_fwd(y, g, g, torch.zeros_like(g), g.clone(), None, False, 0.1, 1e-5, SLOPE, 0.5, 7, None)
    b = ops.bn_act_fwd(y, g, g, torch.zeros_like(g), g.clone(), None, False, 0.1, 1e-5, SLOPE, 0.0, 0, None)
    assert torch.equal(a[0], b[0])


def test_bn_act_generated_mask_is_the_dropout_generator(lib, ops):
    """With a null mask and a seed the kept set is what ops.dropout of a ones tensor gives for that seed, forward and backward."""
    ck = R.Checker()
    for dt in DT:
        for M, C, pd, seed in ((256, 96, 0.05, 11), (1369, 200, 0.5, 0x1234567890ABCDEF), (5, 8, 0.5, 3)):
            ctx = f"{dt} M={M} C={C} p={pd} seed={seed}"
            y, dout, scale, shift, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=M)
            beta = UR.rnd(C, seed=1, scale=0.1)
            yd = up(y).view(1, 1, M, C)
            ones = torch.ones(M * C, dtype=dt, device=dev())
            kept = torch.empty_like(ones)
            ops.dropout(ones, kept, pd, seed)
            keep = (kept != 0).to(torch.uint8).view(1, 1, M, C)
            assert 0 < int(keep.sum()) < M * C
            a = ops.bn_act_fwd(yd, up(gamma), up(beta), None, None, None, True, 0.1, 1e-5, SLOPE, pd, seed, None)
            b = ops.bn_act_fwd(yd, up(gamma), up(beta), None, None, None, True, 0.1, 1e-5, SLOPE, pd, 0, keep)
            ck.exact("generated mask forward", a[0], b[0], ctx)
            if bool(((a[0] != 0) != (keep != 0)).any()):
                ck.fail("generated mask forward", ctx, "the non-zero outputs are not the kept set")
            dd = up(dout).view(1, 1, M, C)
            ga = ops.bn_act_bwd(yd, dd, a[3], a[4], a[1], a[2], up(gamma), SLOPE, pd, seed, None)
            gb = ops.bn_act_bwd(yd, dd, a[3], a[4], a[1], a[2], up(gamma), SLOPE, pd, 0, keep)
            for u, v in zip(ga, gb):
                ck.exact("generated mask backward", u, v, ctx)
    finish(ck)


def test_bn_act_without_slope_and_dropout_is_bn_relu(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, (M, C) in enumerate(((2, 1), (257, 96), (1369, 257), (255, 520))):
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i, mean=0.3)
            yd = up(y).view(1, 1, M, C)
            for training in (True, False):
                ctx = f"{dt} M={M} C={C} training={training}"
                bufs = [(up(rm), up(rv), torch.zeros((), dtype=torch.int64, device=dev())) for _ in range(2)]
                a = ops.bn_fwd(yd, up(gamma), up(beta), *bufs[0], training, 0.1, 1e-5, relu=True)
                b = ops.bn_act_fwd(yd, up(gamma), up(beta), *bufs[1], training, 0.1, 1e-5, 0.0, 0.0, 0, None)
                for u, v in zip(a, b):
                    if u is not None:
                        ck.exact("bn_act(slope 0, p 0) == bn+relu", v, u, ctx)
                for u, v in zip(*bufs):
                    ck.exact("bn_act(slope 0, p 0) buffers", v, u, ctx)
                if training:
                    dout = up(UR.rnd(M, C, seed=i + 9).to(dt)).view(1, 1, M, C)
                    ga = ops.bn_relu_bwd(yd, dout, a[3], a[4], a[1], a[2], up(gamma))
                    gb = ops.bn_act_bwd(yd, dout, a[3], a[4], a[1], a[2], up(gamma), 0.0, 0.0, 0, None)
                    for u, v in zip(ga, gb):
                        ck.exact("bn_act_bwd(slope 0, p 0) == bn_relu_bwd", v, u, ctx)
    finish(ck)


def test_bn_act_refuses_bad_dropout_arguments(lib, ops):
    from uia_hip._lib import UiaError
    y = torch.zeros(1, 1, 4, 8, dtype=F32, device=dev())
    g = torch.ones(8, dtype=F32, device=dev())
    for pd in (1.0, 1.5, -0.1):
        with pytest.raises(UiaError, match="drop_p"):
            ops.bn_act_fwd(y, g, g, None, None, None, True, 0.1, 1e-5, SLOPE, pd, 0, None)
        out = Out((4, 8), F32)
        assert lib.uia_bn_act_fwd(ops._stream(), ops._code(F32), 1, 4, 8, y.data_ptr(), g.data_ptr(), g.data_ptr(), None, None, None, 0.1, 1e-5, g.data_ptr(),
                                  g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), SLOPE, p(out), pd, 0, None) != 0
        assert out.intact() and bool(torch.isnan(out.t).all())
    with pytest.raises(UiaError, match="keep_mask"):
        ops.bn_act_fwd(y, g, g, None, None, None, True, 0.1, 1e-5, SLOPE, 0.5, 0, torch.ones(1, 1, 4, 7, dtype=torch.uint8, device=dev()))
    with pytest.raises(UiaError, match="multiple of 8"):
        ops.bn_act_fwd(torch.zeros(1, 1, 3, 5, dtype=F32, device=dev()), g[:5].contiguous(), g[:5].contiguous(), None, None, None, True, 0.1, 1e-5, SLOPE, 0.5, 7, None)
