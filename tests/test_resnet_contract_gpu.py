"""-m gpu: what the kernels the ResNet baseline added must compute, element by element against the float64 restatements of
tests/resnet_reference.py on the operands the kernel sees, in both dtypes: the strided convolution (csrc/unet_conv.hip: forward, data
gradient, weight gradient, k in {1, 3, 7} x s in {1, 2}, both kernel forms), the packed stem, MaxPool2d(3, 2, 1) (csrc/unet_pool.hip, exact),
BatchNorm + add + ReLU (csrc/unet_bn.hip), the global average pool, the layout helper and the two-tensor add.  The bounds are those of
tests/unet_reference.py (c_conv, c_wgrad, c_reduce) at each case's own K and M.

As in tests/test_unet_baseline_contract_gpu.py every output and scratch buffer is a view inside a NaN-filled buffer with guard elements on
both sides, the calls go to the C entry points, and each case also runs through its uia_hip.ops wrapper, whose result must be bit-identical."""
import pytest
import torch

import helpers_reference as R
import resnet_reference as RR
import unet_baseline_reference as UB
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


def up_off(t):
    """The same values one element into a device buffer: contiguous, and not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=dev())
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


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


# ------------------------------------------------------------------------------------------ strided convolution
def conv_case(lib, ops, ck, dt, B, H, W, C, N, k, s, seed, place=up, seen=None):
    """Forward, data gradient and weight gradient of one geometry against float64; `place` puts the operands on the device."""
    Ho, Wo = RR.out_hw(H, W, s)
    K = k * k * C
    x = UR.rnd(B, H, W, C, seed=seed).to(dt)
    w = UR.rnd(N, K, seed=seed + 100, scale=K ** -0.5).to(dt)
    dy = UR.rnd(B, Ho, Wo, N, seed=seed + 200).to(dt)
    wd = RR.dgrad_rows(w, k, C)
    xd, wdev, dyd, wdd = place(x), place(w), place(dy), place(wd)
    code, st = ops._code(dt), ops._stream()
    ctx = f"{dt} B={B} {H}x{W} C={C} N={N} k={k} s={s} {place.__name__}"

    ref, mag = RR.conv_strided(x, w, k, s)
    y = Out((B, Ho, Wo, N), dt)
    if call(ck, ctx, "uia_conv_strided", lib.uia_conv_strided(st, code, 0, B, H, W, C, k, s, p(xd), N, p(wdev), p(y))):
        ck.check(bar("strided forward", dt), y.t, ref, R.bound(ref, mag, UR.c_conv(k * k, C), dt), ctx)
        ck.exact("wrapper", ops.conv_strided(xd, wdev, N, k, s), y.t, ctx)
        guards(ck, "guards", ctx, y)

    ref, mag = RR.conv_strided_dgrad(dy, wd, (H, W), k, s)
    dx = Out((B, H, W, C), dt)
    if call(ck, ctx + " dgrad", "uia_conv_strided", lib.uia_conv_strided(st, code, 1, B, H, W, C, k, s, p(dyd), N, p(wdd), p(dx))):
        ck.check(bar("strided dgrad", dt), dx.t, ref, R.bound(ref, mag, UR.c_conv(k * k, N), dt), ctx)
        ck.exact("wrapper", ops.conv_strided_dgrad(dyd, wdd, (H, W), C, k, s), dx.t, ctx)
        guards(ck, "guards", ctx, dx)

    ref, mag = RR.conv_strided_wgrad(x, dy, k, s)
    S = lib.uia_conv_strided_wgrad_splits(B, H, W, C, k, s, N)
    if seen is not None:
        seen.add(S)
    got = []
    for _ in range(2):
        ws = Out((S * N * K,), F32) if S > 1 else None
        dw = Out((N, K), F32)
        if not call(ck, ctx + " wgrad", "uia_conv_strided_wgrad", lib.uia_conv_strided_wgrad(st, code, B, H, W, C, k, s, p(xd), N, p(dyd), p(ws), p(dw))):
            return
        guards(ck, "guards", ctx, dw, *([ws] if ws else []))
        got.append(dw)
    ck.exact("wgrad deterministic", got[1].t, got[0].t, ctx)
    ck.exact("wrapper", ops.conv_strided_wgrad(xd, dyd, k, s), got[0].t, ctx)
    ck.check("strided wgrad", got[0].t, ref, R.bound(ref, mag, UR.c_wgrad(B * Ho * Wo, S)), ctx + f" splits={S}")


@pytest.mark.parametrize("k, s", RR.KS)
def test_strided_conv_on_the_matrix_cores(lib, ops, k, s):
    ck, seen = R.Checker(), set()
    for dt in DT:
        for gi, (H, W) in enumerate(RR.GRIDS):
            for ci, (C, N) in enumerate(RR.CONV_CN):
                assert ops.conv_strided_form(0, C, N, k, s) == 1 and ops.conv_strided_form(1, C, N, k, s) == 1 and ops.conv_strided_wgrad_form(C, N, k, s) == 1
                conv_case(lib, ops, ck, dt, 2, H, W, C, N, k, s, 1000 + 100 * k + 10 * gi + ci, seen=seen)
    finish(ck)
    # the weight gradient ran at one pixel range (the 18- or 24-pixel grids of stride 2; 60 pixels otherwise give two) and at more than one
    assert max(seen) > 1 and (s == 1 or min(seen) == 1), seen


@pytest.mark.parametrize("k, s", RR.KS)
def test_strided_conv_direct_form(lib, ops, k, s):
    """C = 3 and N = 2, and matrix-core shapes whose operands sit one element into their buffer."""
    ck = R.Checker()
    for dt in DT:
        for gi, (H, W) in enumerate(RR.GRIDS):
            for C, N in RR.CONV_DIRECT_CN:
                assert ops.conv_strided_form(0, C, N, k, s) == 0 and ops.conv_strided_wgrad_form(C, N, k, s) == 0
                conv_case(lib, ops, ck, dt, 2, H, W, C, N, k, s, 2000 + 100 * k + 10 * gi)
        conv_case(lib, ops, ck, dt, 2, 7, 10, 8, 8, k, s, 2500 + k, place=up_off)
        conv_case(lib, ops, ck, dt, 2, 5, 6, 40, 72, k, s, 2600 + k, place=up_off)
    finish(ck)


def test_weight_gradient_at_one_and_at_several_splits(lib, ops):
    ck, seen = R.Checker(), set()
    for dt in DT:
        conv_case(lib, ops, ck, dt, 1, 4, 4, 8, 8, 3, 1, 2700, seen=seen)          # 16 pixels: one range
        conv_case(lib, ops, ck, dt, 2, 16, 18, 8, 16, 3, 2, 2701, seen=seen)       # 144 pixels: five ranges of 32
    finish(ck)
    assert min(seen) == 1 and max(seen) > 1, seen


def test_packed_stem_is_the_three_channel_convolution(lib, ops):
    """The 7x7 stride-2 stem with its 3 channels in 8: image and weight packed by uia_nchw_to_nhwc, against the 3-channel float64 conv on the
    operands rounded to the compute dtype; the weight gradient's pad columns are zeros and the rest is the 3-channel gradient."""
    ck = R.Checker()
    B, H, W, N = 2, 18, 21, 64
    Ho, Wo = RR.out_hw(H, W, 2)
    for dt in DT:
        for cin in (3, 1):
            ctx = f"{dt} stem from {cin} channel(s)"
            img = UR.rnd(B, cin, H, W, seed=31 + cin)
            w = UR.rnd(N, 3, 7, 7, seed=41, scale=147 ** -0.5)
            assert ops.conv_strided_form(0, 8, N, 7, 2) == 1 and ops.conv_strided_wgrad_form(8, N, 7, 2) == 1
            xo = Out((B, H, W, 8), dt)
            if not call(ck, ctx, "uia_nchw_to_nhwc", lib.uia_nchw_to_nhwc(ops._stream(), ops._code(dt), B, cin, H, W, 8, 3, p(up(img)), p(xo))):
                continue
            ck.exact("packed image", xo.t, RR.pack_image(img, dt), ctx)
            ck.exact("wrapper", ops.nchw_to_nhwc(up(img), 8, 3, dt), xo.t, ctx)
            w8 = torch.zeros(N, 7, 7, 8, dtype=dt)
            w8[..., :3] = w.permute(0, 2, 3, 1).to(dt)
            wo = Out((N, 7, 7, 8), dt)
            if not call(ck, ctx, "uia_nchw_to_nhwc", lib.uia_nchw_to_nhwc(ops._stream(), ops._code(dt), N, 3, 7, 7, 8, 3, p(up(w)), p(wo))):
                continue
            ck.exact("packed weight", wo.t, w8, ctx)
            guards(ck, "guards", ctx, xo, wo)
            x3 = img.expand(-1, 3, -1, -1).permute(0, 2, 3, 1).to(dt).contiguous()          # NHWC, 3 channels, rounded
            w3 = w.permute(0, 2, 3, 1).to(dt).reshape(N, 147)
            ref, mag = RR.conv_strided(x3, w3, 7, 2)
            y = ops.conv_strided(xo.t, wo.t.view(N, 392), N, 7, 2)
            ck.check(bar("stem forward", dt), y, ref, R.bound(ref, mag, UR.c_conv(49, 8), dt), ctx)
            dy = UR.rnd(B, Ho, Wo, N, seed=51).to(dt)
            ref, mag = RR.conv_strided_wgrad(x3, dy, 7, 2)
            dw = ops.conv_strided_wgrad(xo.t, up(dy), 7, 2).view(N, 49, 8)
            S = lib.uia_conv_strided_wgrad_splits(B, H, W, 8, 7, 2, N)
            ck.check("stem wgrad", dw[..., :3].contiguous(), ref, R.bound(ref, mag, UR.c_wgrad(B * Ho * Wo, S)), ctx + f" splits={S}")
            if bool((dw[..., 3:] != 0).any()):
                ck.fail("stem wgrad", ctx, "a pad column of the weight gradient is not zero")
    finish(ck)


def test_strided_conv_refusals_touch_no_output(lib, ops):
    from uia_hip._lib import UiaError
    for dt in DT:
        x = torch.zeros(1, 4, 4, 8, dtype=dt, device=dev())
        w = torch.zeros(8, 25 * 8, dtype=dt, device=dev())
        code, st = ops._code(dt), ops._stream()
        y, dw = Out((1, 4, 4, 8), dt), Out((8, 25 * 8), F32)
        for k, s, word in ((5, 1, b"kernel size"), (3, 3, b"stride")):
            assert lib.uia_conv_strided(st, code, 0, 1, 4, 4, 8, k, s, x.data_ptr(), 8, w.data_ptr(), p(y)) != 0
            assert word in lib.uia_last_error()
            assert lib.uia_conv_strided(st, code, 1, 1, 4, 4, 8, k, s, x.data_ptr(), 8, w.data_ptr(), p(y)) != 0
            assert lib.uia_conv_strided_wgrad(st, code, 1, 4, 4, 8, k, s, x.data_ptr(), 8, x.data_ptr(), None, p(dw)) != 0
            assert word in lib.uia_last_error()
        assert lib.uia_conv_strided(st, code, 2, 1, 4, 4, 8, 3, 1, x.data_ptr(), 8, w.data_ptr(), p(y)) != 0
        for args in ((None, w.data_ptr(), p(y)), (x.data_ptr(), None, p(y)), (x.data_ptr(), w.data_ptr(), None)):
            assert lib.uia_conv_strided(st, code, 0, 1, 4, 4, 8, 3, 1, args[0], 8, args[1], args[2]) != 0
            assert b"null tensor" in lib.uia_last_error()
        assert lib.uia_conv_strided_wgrad(st, code, 1, 4, 4, 8, 3, 1, None, 8, x.data_ptr(), None, p(dw)) != 0
        assert lib.uia_conv_strided_wgrad(st, code, 1, 4, 4, 8, 3, 1, x.data_ptr(), 8, x.data_ptr(), None, None) != 0
        assert lib.uia_conv_strided(st, code, 0, 0, 4, 4, 8, 3, 1, x.data_ptr(), 8, w.data_ptr(), p(y)) != 0
        torch.cuda.synchronize()
        assert y.intact() and dw.intact() and bool(torch.isnan(y.t).all()) and bool(torch.isnan(dw.t).all())
        with pytest.raises(UiaError, match="not built"):
            ops.conv_strided(x, w, 8, 5, 1)
        with pytest.raises(UiaError, match="not built"):
            ops.conv_strided_wgrad(x, x, 3, 3)


# ------------------------------------------------------------------------------------------ max-pool 3 / 2 / 1
def pool_case(lib, ops, ck, ctx, dt, x, xd):
    B, H, W, C = x.shape
    Ho, Wo = RR.out_hw(H, W, 2)
    ref, _ = RR.maxpool3s2(x)
    y = Out((B, Ho, Wo, C), dt)
    if not call(ck, ctx, "uia_maxpool3s2_fwd", lib.uia_maxpool3s2_fwd(ops._stream(), ops._code(dt), B, H, W, C, xd.data_ptr(), p(y))):
        return
    ck.exact("maxpool forward", y.t, ref.to(dt), ctx)
    ck.exact("wrapper", ops.maxpool3s2(xd), y.t, ctx)
    dy = UR.rnd(B, Ho, Wo, C, seed=B + H + W + C).to(dt)
    dyd = up(dy)
    dx = Out((B, H, W, C), dt)
    if not call(ck, ctx, "uia_maxpool3s2_bwd", lib.uia_maxpool3s2_bwd(ops._stream(), ops._code(dt), B, H, W, C, xd.data_ptr(), p(dyd), p(dx))):
        return
    if bool(torch.isnan(dx.t).any()):
        ck.fail("maxpool backward", ctx, "dx holds NaN: an element was not written")
    ck.exact("maxpool backward", dx.t, RR.maxpool3s2_bwd(x, dy, acc=F32).to(dt), ctx)
    ck.exact("wrapper", ops.maxpool3s2_bwd(xd, dyd), dx.t, ctx)
    guards(ck, "guards", ctx, y, dx)


def test_maxpool3s2_forward_backward_exact(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, (H, W) in enumerate(RR.POOL_HW):
            for C in RR.POOL_C:
                for j, kind in enumerate(RR.POOL_DATA):
                    x = RR.pool_data(kind, (2, H, W, C), dt, 10 * i + j)
                    pool_case(lib, ops, ck, f"{dt} {H}x{W} C={C} {kind}", dt, x, up(x))
                    if kind in ("random", "ties"):
                        pool_case(lib, ops, ck, f"{dt} {H}x{W} C={C} {kind} one element into its buffer", dt, x, up_off(x))
        x = RR.pool_data("negative", (1, 7, 9, 8), dt, 99)
        assert float(RR.maxpool3s2(x)[0].max()) < 0          # a zero padding would have won every border window
    finish(ck)


def test_maxpool3s2_refusals(lib, ops):
    for dt in DT:
        x = torch.zeros(1, 4, 4, 8, dtype=dt, device=dev())
        y, dx = Out((1, 2, 2, 8), dt), Out((1, 4, 4, 8), dt)
        assert lib.uia_maxpool3s2_fwd(ops._stream(), ops._code(dt), 1, 4, 4, 8, None, p(y)) != 0 and b"null tensor" in lib.uia_last_error()
        assert lib.uia_maxpool3s2_fwd(ops._stream(), ops._code(dt), 1, 0, 4, 8, x.data_ptr(), p(y)) != 0
        assert lib.uia_maxpool3s2_bwd(ops._stream(), ops._code(dt), 1, 4, 4, 8, x.data_ptr(), None, p(dx)) != 0
        torch.cuda.synchronize()
        assert y.intact() and dx.intact() and bool(torch.isnan(y.t).all()) and bool(torch.isnan(dx.t).all())


# ------------------------------------------------------------------------------------------ BatchNorm + add + ReLU
def bn_grid():
    i = 0
    for C in RR.BN_C:
        for M in RR.BN_M:
            yield i, M, C
            i += 1


def test_bn_add_relu_forward(lib, ops):
    ck = R.Checker()
    eps, mom = UR.f32(1e-5), 0.1
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i, mean=0.3)
            r = UR.rnd(M, C, seed=40 + i).to(dt)
            yd, rd, gd, bd = up(y), up(r), up(gamma), up(beta)
            c = UR.c_reduce(M, C) + RR.C_ADD
            ctx = f"{dt} M={M} C={C}"
            ref = RR.bn_add_relu_train(y, r, gamma, beta, rm, rv, 0, UR.f32(mom), eps)
            rmo, rvo = Out((C,), F32, init=rm), Out((C,), F32, init=rv)
            nbt = torch.zeros(1, dtype=torch.int64, device=dev())
            ws = Out((UR.bn_slices(M) * C * 3,), F32)
            mean, invstd, scale, shift, out = Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt)
            if not call(ck, ctx, "uia_bn_add_relu_fwd", lib.uia_bn_add_relu_fwd(ops._stream(), ops._code(dt), 1, M, C, p(yd), p(rd), p(gd), p(bd), p(rmo), p(rvo),
                                                                                nbt.data_ptr(), mom, eps, p(ws), p(mean), p(invstd), p(scale), p(shift), p(out))):
                continue
            for k, o in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift), ("run_mean", rmo), ("run_var", rvo)):
                ck.check("bn_add_relu " + k, o.t, ref[k][0], R.bound(ref[k][0], ref[k][1], c), ctx)
            ck.check(bar("bn_add_relu out", dt), out.t, ref["out"][0], R.bound(ref["out"][0], ref["out"][1], c, dt), ctx)
            if int(nbt) != 1:
                ck.fail("bn_add_relu num_batches_tracked", ctx, f"{int(nbt)}")
            guards(ck, "guards", ctx, ws, mean, invstd, scale, shift, out, rmo, rvo)
            rm2, rv2, nbt2 = up(rm), up(rv), torch.zeros((), dtype=torch.int64, device=dev())
            got = ops.bn_add_relu_fwd(yd.view(1, 1, M, C), rd.view(1, 1, M, C), gd, bd, rm2, rv2, nbt2, True, mom, eps)
            for g, o in zip(got, (out, mean, invstd, scale, shift)):
                ck.exact("wrapper", g, o.t, ctx)
            ck.exact("wrapper", rm2, rmo.t, ctx)
            ck.exact("wrapper", rv2, rvo.t, ctx)
            # eval mode: the running statistics, buffers untouched
            ref, mag = RR.bn_add_relu_eval(y, r, gamma, beta, rm, rv, eps)
            ev = ops.bn_add_relu_fwd(yd.view(1, 1, M, C), rd.view(1, 1, M, C), gd, bd, up(rm), up(rv), None, False, mom, eps)
            ck.check(bar("bn_add_relu eval", dt), ev[0], ref, R.bound(ref, mag, UR.C_BN_EVAL + RR.C_ADD, dt), ctx)
    finish(ck)


def test_bn_add_relu_without_r_is_bn_relu_and_slope_one_is_plain_bn(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            y, gamma, beta, rm, rv = UR.bn_case(M, C, dt, seed=i, mean=0.3)
            yd = up(y).view(1, 1, M, C)
            for training in (True, False):
                ctx = f"{dt} M={M} C={C} training={training}"
                bufs = [(up(rm), up(rv), torch.zeros((), dtype=torch.int64, device=dev())) for _ in range(2)]
                a = ops.bn_fwd(yd, up(gamma), up(beta), *bufs[0], training, 0.1, 1e-5, relu=True)
                b = ops.bn_add_relu_fwd(yd, None, up(gamma), up(beta), *bufs[1], training, 0.1, 1e-5)
                for u, v in zip(a, b):
                    if u is not None:
                        ck.exact("bn_add_relu(r null) == bn+relu", v, u, ctx)
                for u, v in zip(*bufs):
                    ck.exact("bn_add_relu(r null) buffers", v, u, ctx)
                # the downsample branch: slope 1, no dropout is BatchNorm with no activation
                a = ops.bn_fwd(yd, up(gamma), up(beta), up(rm), up(rv), None, training, 0.1, 1e-5, relu=False)
                b = ops.bn_act_fwd(yd, up(gamma), up(beta), up(rm), up(rv), None, training, 0.1, 1e-5, 1.0, 0.0, 0, None)
                for u, v in zip(a, b):
                    if u is not None:
                        ck.exact("bn_act(slope 1) == plain bn", v, u, ctx)
            # and its backward is the BatchNorm backward on dout itself
            yb, dout, scale, shift, mean, invstd, gamma_b = UR.bn_bwd_case(M, C, dt, seed=i)
            ones = torch.ones_like(yb, dtype=F32).to(dt)
            want = RR.bn_add_relu_bwd(yb, ones, dout, mean, invstd, gamma_b)
            got = ops.bn_act_bwd(up(yb).view(1, 1, M, C), up(dout).view(1, 1, M, C), up(scale), up(shift), up(mean), up(invstd), up(gamma_b), 1.0, 0.0, 0, None)
            c = UR.c_reduce(M, C) + UB.C_ACT
            ck.check(bar("bn_act(slope 1) bwd dy", dt), got[0], want["dy"][0], R.bound(want["dy"][0], want["dy"][1], c, dt), f"{dt} M={M} C={C}")
            ck.check("bn_act(slope 1) bwd dgamma", got[1], want["dgamma"][0], R.bound(want["dgamma"][0], want["dgamma"][1], c), f"{dt} M={M} C={C}")
            ck.check("bn_act(slope 1) bwd dbeta", got[2], want["dbeta"][0], R.bound(want["dbeta"][0], want["dbeta"][1], c), f"{dt} M={M} C={C}")
    finish(ck)


def test_bn_add_relu_backward(lib, ops):
    """out is the forward's output: about half of its elements are exact zeros (and take no gradient), the rest positive."""
    ck = R.Checker()
    for dt in DT:
        for i, M, C in bn_grid():
            y, dout, _, _, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=i)
            out = torch.relu(UR.rnd(M, C, seed=60 + i)).to(dt)
            assert 0.3 < float((out == 0).float().mean()) < 0.7
            ctx = f"{dt} M={M} C={C}"
            ref = RR.bn_add_relu_bwd(y, out, dout, mean, invstd, gamma)
            dev_in = [up(t) for t in (y, out, dout, mean, invstd, gamma)]
            c = UR.c_reduce(M, C) + RR.C_ADD
            ws, dgamma, dbeta, dy, dr = Out((UR.bn_slices(M) * C * 3,), F32), Out((C,), F32), Out((C,), F32), Out((M, C), dt), Out((M, C), dt)
            if not call(ck, ctx, "uia_bn_add_relu_bwd", lib.uia_bn_add_relu_bwd(ops._stream(), ops._code(dt), M, C, *(p(t) for t in dev_in), p(ws), p(dgamma), p(dbeta),
                                                                                p(dy), p(dr))):
                continue
            ck.check(bar("bn_add_relu bwd dy", dt), dy.t, ref["dy"][0], R.bound(ref["dy"][0], ref["dy"][1], c, dt), ctx)
            ck.check("bn_add_relu bwd dgamma", dgamma.t, ref["dgamma"][0], R.bound(ref["dgamma"][0], ref["dgamma"][1], c), ctx)
            ck.check("bn_add_relu bwd dbeta", dbeta.t, ref["dbeta"][0], R.bound(ref["dbeta"][0], ref["dbeta"][1], c), ctx)
            ck.exact("bn_add_relu bwd dr", dr.t, ref["dr"].to(dt), ctx)
            guards(ck, "guards", ctx, ws, dgamma, dbeta, dy, dr)
            v = [t.view(1, 1, M, C) for t in dev_in[:3]]
            got = ops.bn_add_relu_bwd(*v, *dev_in[3:])
            for g, o in zip(got, (dy, dr, dgamma, dbeta)):
                ck.exact("wrapper", g, o.t, ctx)
            # a null dr is allowed and changes nothing else
            got = ops.bn_add_relu_bwd(*v, *dev_in[3:], want_dr=False)
            assert got[1] is None
            ck.exact("dr null", got[0], dy.t, ctx)
    finish(ck)


def test_relu_gates_select_and_do_not_multiply(ops):
    """Where its gate is closed (z <= 0 for bn_relu_bwd, out == 0 for bn_add_relu_bwd) a ReLU backward never reads dout: with +inf there
    dgamma, dbeta and dy are finite and the bits of the same call with 0 there, and dr is 0.  A gate that multiplied dout by 0 would give NaN."""
    M, C = 8, 8
    for dt in DT:
        y, dout, scale, shift, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=5)
        out = torch.relu(UR.rnd(M, C, seed=65)).to(dt)
        z = torch.addcmul(shift, y.float(), scale)                      # y is clear of the band around z == 0, so fp32 decides as the kernel does
        v4 = lambda t: up(t).view(1, 1, M, C)                           # noqa: E731
        bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)   # noqa: E731
        stats = [up(t) for t in (mean, invstd, gamma)]
        for name, closed in (("bn_relu_bwd", z <= 0), ("bn_add_relu_bwd", out == 0)):
            assert 0 < int(closed.sum()) < M * C
            got = []
            for fill in (float("inf"), 0.0):
                d = torch.where(closed, torch.full_like(dout, fill), dout)
                if name == "bn_relu_bwd":
                    dy, dgamma, dbeta = ops.bn_relu_bwd(v4(y), v4(d), up(scale), up(shift), *stats)
                    dr = None
                else:
                    dy, dr, dgamma, dbeta = ops.bn_add_relu_bwd(v4(y), v4(out), v4(d), *stats)
                got.append((dy, dgamma, dbeta, dr))
            for k, a, b in zip(("dy", "dgamma", "dbeta"), got[0], got[1]):
                assert bool(torch.isfinite(a).all()), f"{name} {dt}: {k} is not finite beside a closed gate"
                assert torch.equal(bits(a), bits(b)), f"{name} {dt}: {k} depends on dout behind a closed gate"
            if name == "bn_add_relu_bwd":
                assert torch.equal(bits(got[0][3]), bits(got[1][3])) and bool((got[0][3].view(M, C)[up(closed)] == 0).all()), f"{name} {dt}: dr behind a closed gate"


def test_bn_add_relu_refusals(lib, ops):
    y = torch.zeros(4, 8, dtype=F32, device=dev())
    g = torch.ones(8, dtype=F32, device=dev())
    out, dg = Out((4, 8), F32), Out((8,), F32)
    st, code = ops._stream(), ops._code(F32)
    assert lib.uia_bn_add_relu_fwd(st, code, 0, 4, 8, y.data_ptr(), None, g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), None, 0.1, 1e-5, None, None, None,
                                   g.data_ptr(), None, p(out)) != 0
    assert b"null tensor" in lib.uia_last_error()
    assert lib.uia_bn_add_relu_bwd(st, code, 4, 8, y.data_ptr(), None, y.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), None, p(dg), p(dg), p(out), None) != 0
    assert b"null tensor" in lib.uia_last_error()
    torch.cuda.synchronize()
    assert out.intact() and dg.intact() and bool(torch.isnan(out.t).all())


# ------------------------------------------------------------------------------------------ average pool, add
def test_avgpool_forward_backward(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for H, W in RR.AVG_HW:
            for C in RR.AVG_C:
                B = 3
                ctx = f"{dt} {H}x{W} C={C}"
                x = UR.rnd(B, H, W, C, seed=H + C, shift=0.5).to(dt)
                ref, mag = RR.avgpool(x)
                o = Out((B, C), F32)
                if not call(ck, ctx, "uia_avgpool_fwd", lib.uia_avgpool_fwd(ops._stream(), ops._code(dt), B, H, W, C, p(up(x)), p(o))):
                    continue
                ck.check("avgpool forward", o.t, ref, R.bound(ref, mag, RR.c_avgpool(H * W)), ctx)
                ck.exact("wrapper", ops.avgpool(up(x)), o.t, ctx)
                g = UR.rnd(B, C, seed=H + C + 1)
                ref, mag = RR.avgpool_bwd(g, (H, W))
                dx = Out((B, H, W, C), dt)
                if not call(ck, ctx, "uia_avgpool_bwd", lib.uia_avgpool_bwd(ops._stream(), ops._code(dt), B, H, W, C, p(up(g)), p(dx))):
                    continue
                ck.check(bar("avgpool backward", dt), dx.t, ref, R.bound(ref, mag, 2, dt), ctx)
                ck.exact("wrapper", ops.avgpool_bwd(up(g), (H, W), dt), dx.t, ctx)
                guards(ck, "guards", ctx, o, dx)
    finish(ck)
    x = torch.zeros(1, 2, 2, 8, dtype=F32, device=dev())
    o = Out((1, 8), F32)
    assert lib.uia_avgpool_fwd(ops._stream(), ops._code(F32), 1, 2, 2, 8, None, p(o)) != 0 and b"null tensor" in lib.uia_last_error()
    assert lib.uia_avgpool_fwd(ops._stream(), ops._code(F32), 1, 0, 2, 8, x.data_ptr(), p(o)) != 0
    torch.cuda.synchronize()
    assert o.intact() and bool(torch.isnan(o.t).all())


def test_add2_is_one_rounded_sum(lib, ops):
    ck = R.Checker()
    for dt in DT:
        for n, place in ((8 * 37, up), (13, up), (8 * 5, up_off)):
            a, b = UR.rnd(n, seed=n).to(dt), UR.rnd(n, seed=n + 1).to(dt)
            ctx = f"{dt} n={n} {place.__name__}"
            o = Out((n,), dt)
            ad, bd = place(a), place(b)
            if not call(ck, ctx, "uia_add2", lib.uia_add2(ops._stream(), ops._code(dt), n, p(ad), p(bd), p(o))):
                continue
            ck.exact("add2", o.t, (a.float() + b.float()).to(dt), ctx)
            ck.exact("wrapper", ops.add2(ad, bd), o.t, ctx)
            guards(ck, "guards", ctx, o)
    finish(ck)
