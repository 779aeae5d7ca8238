"""The per-kernel float64 restatements of tests/unet_reference.py against PyTorch's own float64 ops and their autograd (F.conv2d,
F.conv_transpose2d, F.batch_norm, F.interpolate), at the shapes tests/test_unet_contract_gpu.py runs.  This is what makes the GPU bars
mean something: the restatements are written from the kernels' layouts, PyTorch's ops from its own.

Bar: |restatement − torch| ≤ 1e-12·mag per element.  This departs from "1e-12 relative per element" read as relative to |ref|: mag is the
restatement's own magnitude (the sum of the absolute values of the element's terms), the scale against which two float64 sums of those terms
in different orders differ by a few 1e-16; an element whose terms cancel to 1e-5 of mag would miss 1e-12·|ref| with both sides right.  Every mag is ≥ |ref| element-wise, and no BatchNorm
backward case of the GPU test has an element in the ambiguous ReLU band."""
import torch
import torch.nn.functional as F

import unet_reference as UR

F64 = torch.float64
TOL = 1e-12


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def close(a, b, mag, what):
    a, b, mag = a.to(F64), b.to(F64), mag.to(F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert bool((mag >= a.abs() * (1 - 1e-12)).all()), f"{what}: mag below |ref|"
    bad = (a - b).abs() > TOL * mag
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, worst {float(((a - b).abs() / mag.clamp_min(1e-300)).max()):.3g}"


def test_conv3x3_restatements_match_conv2d_and_its_autograd():
    for i, (B, H, W, C1, C2, N) in enumerate(UR.CONV_MFMA + UR.CONV_DIRECT):
        Cin = C1 + C2
        x1, x2 = UR.rnd(B, H, W, C1, seed=i).double(), (UR.rnd(B, H, W, C2, seed=i + 50).double() if C2 else None)
        w, bias, dy = UR.rnd(N, 9 * Cin, seed=i + 100).double(), UR.rnd(N, seed=i + 150).double(), UR.rnd(B, H, W, N, seed=i + 200).double()
        x = nchw(x1 if x2 is None else torch.cat([x1, x2], 3)).clone().requires_grad_(True)
        wt = w.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
        y = F.conv2d(x, wt, bias, padding=1)
        y.backward(nchw(dy))
        what = f"conv3x3 {(B, H, W, C1, C2, N)}"
        ref, mag = UR.conv3x3(x1, x2, w, bias)
        close(ref, nhwc(y), mag, what + " forward")
        (r1, r2), (m1, m2) = UR.conv3x3(x1, x2, w, None, n1=1)
        close(torch.cat([r1, r2], 3), nhwc(F.conv2d(x, wt, None, padding=1)), torch.cat([m1, m2], 3), what + " split, no bias")
        ref, mag = UR.conv3x3_dgrad(dy, w)
        close(ref, nhwc(x.grad), mag, what + " dgrad")
        # the data gradient as the kernel runs it: the forward form on dy with the flipped rows, split at C1
        rk, mk = UR.conv3x3(dy, None, UR.conv3_dgrad_rows(w, Cin), None, n1=C1)
        rs, _ = UR.conv3x3_dgrad(dy, w, n1=C1)
        for a, b, m in zip(rk, rs, mk) if C2 else ((rk, rs, mk),):
            close(a, b, m, what + " dgrad rows")
        ref, mag = UR.conv3x3_wgrad(x1, x2, dy)
        close(ref, wt.grad.permute(0, 2, 3, 1).reshape(N, 9 * Cin), mag, what + " wgrad")


def test_convt_restatements_match_conv_transpose2d_and_its_autograd():
    for i, (B, h, w_, Cin, Cout) in enumerate(UR.CONVT):
        x, bias = UR.rnd(B, h, w_, Cin, seed=i).double(), UR.rnd(Cout, seed=i + 50).double()
        rows = UR.rnd(4 * Cout, Cin, seed=i + 100).double()                      # [(2·di + dj)·Cout + o, c]
        dy = UR.rnd(B, 2 * h, 2 * w_, Cout, seed=i + 150).double()
        xq = nchw(x).clone().requires_grad_(True)
        wt = rows.reshape(2, 2, Cout, Cin).permute(3, 2, 0, 1).clone().requires_grad_(True)   # [Cin, Cout, 2, 2]
        y = F.conv_transpose2d(xq, wt, bias, stride=2)
        y.backward(nchw(dy))
        what = f"convt {(B, h, w_, Cin, Cout)}"
        ref, mag = UR.convt_fwd(x, rows, bias)
        close(ref, nhwc(y), mag, what + " forward")
        ref, mag = UR.convt_bwd(dy, rows.T.contiguous())
        close(ref, nhwc(xq.grad), mag, what + " backward")
        ref, mag = UR.convt_wgrad(x, dy)
        close(ref, wt.grad.permute(2, 3, 1, 0).reshape(4 * Cout, Cin), mag, what + " wgrad")


def bn_grid():
    for C in UR.BN_C:
        for M in UR.BN_M:
            yield M, C
    yield UR.BN_CAP


def test_batchnorm_restatements_match_batch_norm_and_its_autograd():
    eps = UR.f32(1e-5)
    for i, (M, C) in enumerate(bn_grid()):
        mom = UR.f32(UR.BN_MOMENTA[i % 3])
        y, gamma, beta, rm, rv = (t.double() for t in UR.bn_case(M, C, torch.float32, seed=i))
        what = f"bn M={M} C={C} momentum={mom}"
        for relu in (True, False):
            r = UR.bn_train(y, gamma, beta, rm, rv, 4, mom, eps, relu=relu)
            rmr, rvr = rm.clone(), rv.clone()
            yq = y.T[None, :, :, None].clone().requires_grad_(True)                  # [1, C, M, 1]
            o = F.batch_norm(yq, rmr, rvr, gamma, beta, training=True, momentum=mom, eps=eps)
            o = torch.relu(o) if relu else o
            close(r["out"][0], o[0, :, :, 0].T, r["out"][1], what + f" out relu={relu}")
            close(r["run_mean"][0], rmr, r["run_mean"][1], what + " running mean")
            close(r["run_var"][0], rvr, r["run_var"][1], what + " running var")
            assert r["nbt"] == 5
            var = y.var(0, unbiased=False)
            close(r["mean"][0], y.mean(0), r["mean"][1], what + " mean")
            close(r["invstd"][0], 1 / torch.sqrt(var + eps), r["invstd"][1], what + " invstd")
            for k in ("scale", "shift"):
                assert bool((r[k][1] >= r[k][0].abs()).all()), what + f" {k}: mag below |ref|"
        assert UR.bn_train(y, gamma, beta, None, None, None, mom, eps)["run_mean"] is None
        ev, mag = UR.bn_eval(y, gamma, beta, rm, rv, eps)
        evr = torch.relu(F.batch_norm(y.T[None, :, :, None], rm.clone(), rv.clone(), gamma, beta, training=False, eps=eps))
        close(ev, evr[0, :, :, 0].T, mag, what + " eval")
        s, mag = UR.colsum(y)
        close(s, y.sum(0), mag, what + " colsum")


def test_batchnorm_backward_restatement_matches_autograd_and_no_case_sits_in_the_relu_band():
    eps = UR.f32(1e-5)
    for dt in (torch.bfloat16, torch.float32):
        for i, (M, C) in enumerate(bn_grid()):
            y, dout, scale, shift, mean, invstd, gamma = UR.bn_bwd_case(M, C, dt, seed=i)
            r = UR.bn_relu_bwd(y, dout, scale, shift, mean, invstd, gamma)
            what = f"bn bwd {dt} M={M} C={C}"
            assert int((r["z"] <= r["band"]).sum()) == 0, what + ": elements in the ambiguous ReLU band"
            for k in ("dy", "dgamma", "dbeta"):
                assert bool((r[k][1] >= r[k][0].abs() * (1 - 1e-12)).all()), what + f" {k}: mag below |ref|"
            # autograd of F.batch_norm + ReLU uses y's own float64 statistics: feed the restatement those instead of the fp32 ones
            yd, g = y.double(), gamma.double()
            beta = UR.bn_case(M, C, dt, seed=i, mean=0.5)[2].double()
            m, var = yd.mean(0), yd.var(0, unbiased=False)
            istd = 1 / torch.sqrt(var + eps)
            sc, sh = g * istd, beta - m * g * istd
            assert not bool(((yd * sc + sh).abs() < 1e-9).any()), what + ": an element at the ReLU's kink under the float64 statistics"
            r = UR.bn_relu_bwd(yd, dout, sc, sh, m, istd, g)
            yq, gq, bq = yd.T[None, :, :, None].clone().requires_grad_(True), g.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            torch.relu(F.batch_norm(yq, None, None, gq, bq, training=True, eps=eps)).backward(dout.double().T[None, :, :, None])
            close(r["dy"][0], yq.grad[0, :, :, 0].T, r["dy"][1], what + " dy")
            close(r["dgamma"][0], gq.grad, r["dgamma"][1], what + " dgamma")
            close(r["dbeta"][0], bq.grad, r["dbeta"][1], what + " dbeta")


def test_tap_matrices_match_interpolate_on_an_identity():
    for n, f in sorted({(s, f) for hw in UR.UPS_HW for s in hw for f in UR.UPS_F}):
        Wm = F.interpolate(torch.eye(n, dtype=F64)[None, None], size=(n * f, n), mode="bilinear", align_corners=True)[0, 0]
        assert float((UR.taps_ac(n, f) - Wm).abs().max()) <= TOL, (n, f)
        assert bool((UR.reach_ac(n, f) >= (Wm != 0).double()).all()), (n, f)
    for n_in, n_out in sorted({(i[a], o[a]) for i, o in UR.AA_SIZES for a in (0, 1)}):
        Wm = F.interpolate(torch.eye(n_in, dtype=F64)[None, None], size=(n_out, n_in), mode="bicubic", antialias=True, align_corners=False)[0, 0]
        assert float((UR.taps_aa(n_in, n_out) - Wm).abs().max()) <= TOL, (n_in, n_out)
    assert torch.equal(UR.taps_aa(7, 7), torch.eye(7, dtype=F64)) and torch.equal(UR.taps_ac(6, 1), torch.eye(6, dtype=F64))


def test_resampling_restatements_match_interpolate_and_its_autograd():
    B = 2
    for f in UR.UPS_F:
        for H, W in UR.UPS_HW:
            for C in UR.UPS_C:
                x = UR.rnd(B, H, W, C, seed=f + H + W).double()
                xq = nchw(x).clone().requires_grad_(True)
                y = F.interpolate(xq, size=(H * f, W * f), mode="bilinear", align_corners=True)
                dy = UR.rnd(B, H * f, W * f, C, seed=f + H).double()
                y.backward(nchw(dy))
                ref, mag = UR.upsample_ac(x, f)
                close(ref, nhwc(y), mag, f"upsample_ac f={f} {H}x{W} C={C} forward")
                ref, mag = UR.upsample_ac(dy, f, backward=True)
                close(ref, nhwc(xq.grad), mag, f"upsample_ac f={f} {H}x{W} C={C} backward")
    for (Hi, Wi), (Ho, Wo) in UR.AA_SIZES:
        for C in UR.AA_C:
            x = UR.rnd(B, Hi, Wi, C, seed=Hi + Wo).double()
            xq = nchw(x).clone().requires_grad_(True)
            y = UR.resize(xq, (Ho, Wo))
            dy = UR.rnd(B, C, Ho, Wo, seed=Hi + Wi).double()
            y.backward(dy)
            ref, mag = UR.resize_aa(x, (Ho, Wo))
            close(ref, y, mag, f"resize_aa {Hi}x{Wi}->{Ho}x{Wo} C={C} forward")
            ref, mag = UR.resize_aa_bwd(dy, (Hi, Wi))
            close(ref, nhwc(xq.grad), mag, f"resize_aa {Hi}x{Wi}->{Ho}x{Wo} C={C} backward")
