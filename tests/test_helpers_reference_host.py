"""Host-only checks of tests/helpers_reference.py (no GPU): each float64 restatement against an independent second form, and the
sensitivity of the bars: the reference's own output with a planted bug must trip the bound the GPU contract tests
(tests/test_helpers_contract_gpu.py) apply to the kernels."""
import math

import pytest
import torch
import torch.nn.functional as F

import helpers_reference as R

F64 = R.F64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def trips(got, ref, bound_):
    c = R.Checker()
    c.check("bar", got, ref, bound_, "planted")
    return not c.ok()


# ------------------------------------------------------------------------------------------ restatements against second forms
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (3, 5)])
@pytest.mark.parametrize("tok_off", [0, 1, 2])
def test_im2col3x3_by_hand_and_col2im_adjoint(hw, tok_off):
    h, w = hw
    B, C = 2, 4
    ntok = tok_off + h * w + 1
    x = rnd(B, ntok, C, seed=h * 10 + w)
    cols = R.im2col3x3(x, h, w, tok_off)
    for b in range(B):
        for y in range(h):
            for xx in range(w):
                for ky in range(3):
                    for kx in range(3):
                        yy, xs = y + ky - 1, xx + kx - 1
                        want = x[b, tok_off + yy * w + xs] if 0 <= yy < h and 0 <= xs < w else torch.zeros(C, dtype=F64)
                        got = cols[(b * h + y) * w + xx, (ky * 3 + kx) * C:(ky * 3 + kx + 1) * C]
                        assert torch.equal(got, want)
    d = rnd(B * h * w, 9 * C, seed=99)
    back = R.col2im3x3(d, B, h, w, C, ntok, tok_off)
    assert math.isclose(float((cols * d).sum()), float((x * back).sum()), rel_tol=1e-12, abs_tol=1e-12)
    assert not back[:, :tok_off].any() and not back[:, tok_off + h * w:].any()


@pytest.mark.parametrize("k1,k2", [(4, 4), (1, 4), (4, 1), (2, 3)])
def test_shuffle_is_inverse_of_unshuffle(k1, k2):
    B, h, w = 2, 3, 2
    ld = k2 * k2 + 3
    tmp = rnd(B * h * w * k1 * k1, ld, seed=k1 * 7 + k2)
    out = R.unshuffle(tmp, B, h, w, k1, k2)
    for (b, y, x, i, j, i2, j2) in [(0, 0, 0, 0, 0, 0, 0), (B - 1, h - 1, w - 1, k1 - 1, k1 - 1, k2 - 1, k2 - 1), (1, 2, 0, k1 // 2, k1 - 1, k2 // 2, 0)]:
        row = ((b * h + y) * w + x) * k1 * k1 + i * k1 + j
        assert out[b, (y * k1 + i) * k2 + i2, (x * k1 + j) * k2 + j2] == tmp[row, i2 * k2 + j2]
    back = R.shuffle(out, B, h, w, k1, k2, ld)
    assert torch.equal(back[:, :k2 * k2], tmp[:, :k2 * k2]) and back[:, k2 * k2:].abs().max() == 0


@pytest.mark.parametrize("hw,HW", [((14, 14), (224, 224)), ((7, 7), (20, 20)), ((1, 1), (5, 5)), ((3, 6), (7, 9)), ((20, 9), (7, 4))])
def test_upsample_hand_taps_and_adjoint(hw, HW):
    img = rnd(2, 3, *hw, seed=hw[0])
    ref = R.upsample(img, *HW)
    assert torch.allclose(R.upsample_taps(img, *HW), ref, rtol=1e-12, atol=1e-12)
    d = rnd(2, 3, *HW, seed=5)
    back = R.upsample_bwd(d, *hw)
    assert math.isclose(float((ref * d).sum()), float((img * back).sum()), rel_tol=1e-10)
    Ry, _ = R.taps_1d(HW[0], hw[0])
    Rx, _ = R.taps_1d(HW[1], hw[1])
    assert torch.allclose(back, Ry.T @ d @ Rx, rtol=1e-12, atol=1e-12)
    assert bool((R.upsample_mag(img, *HW) >= (ref.abs() - 1e-12)).all())


def test_act_bwd_matches_closed_forms():
    x = torch.tensor([0.0, 1e-3, -1e-3, 4.0, -4.0, 30.0, -30.0, 1.0, -1.0], dtype=F64)
    dy = rnd(x.numel(), seed=3)
    phi = torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)
    Phi = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    assert torch.allclose(R.act_bwd(dy, x, "gelu"), dy * (Phi + x * phi), rtol=1e-12, atol=1e-300)
    s = torch.sigmoid(1.702 * x)
    assert torch.allclose(R.act_bwd(dy, x, "quick_gelu"), dy * s * (1 + 1.702 * x * (1 - s)), rtol=1e-12, atol=1e-300)
    assert torch.equal(R.act_bwd(dy, x, "relu"), torch.where(x > 0, dy, torch.zeros_like(dy)))
    assert R.act_bwd(dy, x, "relu")[0] == 0


def test_ln_affine_bwd_matches_closed_form():
    M, D = 5, 12
    x, dy, gamma = rnd(M, D, seed=1) * 3 + 1, rnd(M, D, seed=2), rnd(D, seed=3)
    r = R.ln_affine_bwd(dy, x, gamma, 1e-5)
    mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-5)
    xhat = (x - mu) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    assert torch.allclose(r["dx"], dx, rtol=1e-10, atol=1e-12)
    assert torch.allclose(r["dg"], (dy * xhat).sum(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["db"], dy.sum(0), rtol=1e-12, atol=1e-12)


def test_embed_bwd_and_colsum_and_segment_mean_by_loops():
    ids = torch.tensor([3, 1, 3, 0, 7, -1, 3])
    dx = rnd(7, 4, seed=4)
    out, _ = R.embed_bwd(ids, dx, 5, pad_id=0)
    want = torch.zeros(5, 4, dtype=F64)
    for r in range(7):
        if 0 < ids[r] < 5:
            want[ids[r]] += dx[r]
    assert torch.allclose(out, want, rtol=0, atol=1e-15)
    a = rnd(9, 3, seed=5)
    assert torch.allclose(R.colsum(a)[0], sum(a[m] for m in range(9)), atol=1e-14)
    x = rnd(6, 5, seed=6)
    assert torch.allclose(R.segment_mean(x, 2, 3, 4)[0], torch.stack([x[:3, :4].sum(0) / 3, x[3:, :4].sum(0) / 3]), atol=1e-15)


def test_dicece_gradient_matches_closed_form():
    B, C, H, W = 2, 8, 3, 5
    z = rnd(B, C, H, W, seed=7) * 3
    lab = torch.randint(0, C - 1, (B, 1, H, W), generator=torch.Generator().manual_seed(8)).to(F64)      # class C-1 absent
    loss, dz, mag, _ = R.dicece(z, lab)
    p = torch.softmax(z, 1)
    t = F.one_hot(lab[:, 0].long(), C).permute(0, 3, 1, 2).to(F64)
    I, D = (p * t).sum((2, 3)), (p * p).sum((2, 3)) + t.sum((2, 3)) + 1e-8
    g = (2 / (B * C)) * ((2 * I + 1e-8)[:, :, None, None] * p / (D ** 2)[:, :, None, None] - t / D[:, :, None, None])
    want = p * (g - (g * p).sum(1, keepdim=True)) + (p - t) / (B * H * W)
    assert torch.allclose(dz, want, rtol=1e-10, atol=1e-15)
    assert bool((mag * R.U >= 0).all())


def test_pack_weights_forms_by_reshape():
    src = rnd(5, 7, seed=9)
    RP, CP, g = 8, 9, 4
    out = R.pack_weights(src, 0.5, RP, CP, g, F64)
    assert torch.equal(out["row"].view(RP, CP)[:5, :7], src * 0.5)
    assert torch.equal(out["tr"].view(CP, RP)[:7, :5], (src * 0.5).T)


# ------------------------------------------------------------------------------------------ planted bugs trip the bars
def test_planted_shifted_upsample_tap_is_caught():
    img = rnd(1, 2, 7, 7, seed=11)
    for H, W in ((20, 20), (224, 224)):
        ref = R.upsample(img, H, W)
        shifted = torch.roll(ref, 1, dims=3)                    # every output one pixel to the right
        assert trips(shifted, ref, R.bound(ref, R.upsample_mag(img, H, W), R.C_UPSAMPLE))
        half = R.upsample_taps(img, H, W)
        Rx, _ = R.taps_1d(W, 7)
        Rx2 = torch.zeros_like(Rx)                              # source coordinate + 0.5: the tap shifted by half an input pixel
        for o in range(W):
            s = min(max(7 / W * (o + 0.5) - 0.5, 0.0) + 0.5, 6.0)
            i0 = min(int(s), 6)
            i1 = min(i0 + 1, 6)
            Rx2[o, i0] += 1 - (s - i0)
            Rx2[o, i1] += s - i0
        Ry, _ = R.taps_1d(H, 7)
        assert trips(Ry @ img @ Rx2.T, half, R.bound(half, R.upsample_mag(img, H, W), R.C_UPSAMPLE))


def test_planted_act_bwd_dropped_tail_is_caught():
    x = rnd(21, seed=12) * 4
    dy = rnd(21, seed=13)
    for act in ("gelu", "quick_gelu"):
        ref = R.act_bwd(dy, x, act)
        bad = ref.clone()
        bad[16:] = 0                                            # a vector loop that stops at n - n % 8
        assert trips(bad, ref, R.bound(ref, R.act_bwd_mag(dy, x, act), R.C_ACT_GELU if act == "gelu" else R.C_ACT_QUICK))
        wrong = R.act_bwd(dy, x + 2 ** -10, act)                # the derivative taken at a slightly wrong point
        assert trips(wrong, ref, R.bound(ref, R.act_bwd_mag(dy, x, act), R.C_ACT_GELU if act == "gelu" else R.C_ACT_QUICK))


@pytest.mark.parametrize("M", [3, 5, 4099])
def test_planted_ln_dbeta_without_last_row_is_caught(M):
    D = 8
    x, dy, gamma = rnd(M, D, seed=14), rnd(M, D, seed=15), rnd(D, seed=16)
    r = R.ln_affine_bwd(dy, x, gamma, 1e-5)
    bad = R.ln_affine_bwd(dy[:-1], x[:-1], gamma, 1e-5)
    assert trips(bad["db"], r["db"], R.bound(r["db"], r["mag_db"], R.C_LN))
    dres = rnd(M, D, seed=17)
    with_res = R.ln_affine_bwd(dy, x, gamma, 1e-5, dres)
    assert trips(r["dx"], with_res["dx"], R.bound(with_res["dx"], with_res["mag_dx"], R.C_LN))      # dres dropped


def test_planted_colsum_missing_row_and_segment_off_by_one_are_caught():
    for M in (1, 1023, 1025, 5000):
        a = rnd(M, 70, seed=M)
        ref, mag = R.colsum(a)
        assert trips(ref - a[-1], ref, R.bound(ref, mag, R.C_COLSUM))
    x = rnd(2 * 50, 6, seed=18)
    ref, mag = R.segment_mean(x, 2, 50, 6)
    assert trips(x[:, :6].reshape(2, 50, 6)[:, :49].sum(1) / 50, ref, R.bound(ref, mag, R.C_SEGMENT))


def test_planted_col2im_border_and_film_and_dice_are_caught():
    B, h, w, C = 1, 5, 4, 4
    d = rnd(B * h * w, 9 * C, seed=19)
    ref = R.col2im3x3(d, B, h, w, C, 1 + h * w, 1)
    mag = R.col2im3x3_mag(d, B, h, w, C, 1 + h * w, 1)
    bad = ref.clone()
    bad[0, 1] -= d[0, 0:C]                                      # the corner pixel's kk = 0 slot (outside the grid) is not read ...
    bad[0, 1] += d[1, 0:C]                                      # ... a neighbour's is: the border test of col2im off by one
    assert trips(bad, ref, R.bound(ref, mag, R.C_COL2IM))
    x, dy, mul = rnd(2, 7, 4, seed=20), rnd(2, 7, 4, seed=21), rnd(2, 4, seed=22)
    f = R.film_bwd(dy, x, mul)
    assert trips(f["dmul"] - dy[:, -1] * x[:, -1], f["dmul"], R.bound(f["dmul"], f["mag_dmul"], R.C_FILM))
    z = rnd(2, 3, 4, 4, seed=23)
    lab = torch.randint(0, 3, (2, 1, 4, 4), generator=torch.Generator().manual_seed(24)).to(F64)
    _, dz, mag, _ = R.dicece(z, lab)
    _, dz_wrong, _, _ = R.dicece(z, (lab + 1) % 3)              # labels of the wrong class
    assert trips(dz_wrong, dz, R.bound(dz, mag, R.C_DICE_GRAD))
