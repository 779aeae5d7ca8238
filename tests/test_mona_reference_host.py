"""CPU: the restatements of tests/mona_reference.py against a second form (float64 autograd through oracle/mona_ref.py's literal rfft2 / irfft2,
three conv2d, F.gelu and the keep mask; F.layer_norm for the pre-norm), the closed form of the GELU term against an fp32 emulation of gelu_parts,
the conditions the contract tests' inputs must meet, and planted bugs: each must exceed the bound by 10× somewhere, under the fp32 bound and
under the fast kernel's bound."""
import math

import torch
import torch.nn.functional as F

import mona_reference as MR
from oracle import mona_ref

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
Case = MR.Case
# h = 1, w = 1, hw = 1, non-square grids, a pixel count below the pixel groups, both weight sets, every variant and dropout case
SECOND_FORM = [Case(F32, v, k, 2, h, w, *MR.DROPS[i % 3])
               for i, (v, k, (h, w)) in enumerate([("hybrid", "A", (1, 1)), ("noise_aware", "A", (1, 3)), ("freq_enhanced", "A", (3, 1)), ("baseline", "A", (2, 3)),
                                                   ("hybrid", "Z", (3, 7)), ("hybrid", "A", (5, 4)), ("noise_aware", "A", (1, 4)), ("hybrid", "A", (9, 9)),
                                                   ("freq_enhanced", "A", (6, 14)), ("hybrid", "A", (5, 10))])] + \
              [Case(BF16, "hybrid", "A", 3, 1, 4, *MR.DROPS[1]), Case(BF16, "hybrid", "Z", 2, 5, 14, *MR.DROPS[2])]


def oracle_params(P):
    return {MR.ORACLE_NAMES[k]: v.to(F64).reshape(MR.ORACLE_SHAPES.get(k, v.shape)).clone().requires_grad_(True) for k, v in P.items()}


def autograd_spatial(case):
    t, dd, P, keep = MR.case_inputs(case)
    B, h, w = case.B, case.h, case.w
    tt = t.to(F64).clone().requires_grad_(True)
    Po = oracle_params(P)
    img = tt[:, 1:].reshape(B, h, w, 64).permute(0, 3, 1, 2)
    z_sp = mona_ref.spatial_op(img, Po, case.variant).permute(0, 2, 3, 1).reshape(B, h * w, 64)
    z = torch.cat([tt[:, :1], z_sp], 1)
    d = F.gelu(z)
    if keep is not None:
        d = d * keep.to(F64) / (1.0 - float(torch.tensor(case.p, dtype=F32)))
    d.backward(dd.to(F64))
    grads = {"dt": tt.grad}
    for k in P:
        grads["g_" + k] = Po[MR.ORACLE_NAMES[k]].grad.reshape(P[k].shape)
    return z.detach(), d.detach(), grads


def close(name, ctx, ref, mag, want, tol=1e-11):
    """|ref − want| ≤ tol·mag.  The spatial terms carry their rounding counts inside mag (3 to about 1500 times Σ|terms|), so they are held to 1e-14 of it:
    no looser than 1e-11 of Σ|terms|."""
    worst = float(((ref - want).abs() / (mag + 1e-300)).max())
    assert ref.shape == want.shape and worst <= tol, f"{name}: {ctx}: {worst:.3g} of mag"


def test_spatial_restatement_agrees_with_autograd_through_the_oracle():
    for case in SECOND_FORM:
        ctx = MR.case_name(case)
        t, dd, P, keep = MR.case_inputs(case)
        z, d, grads = autograd_spatial(case)
        fwd = MR.spatial_fwd(case.variant, t, P, case.h, case.w, keep, case.p)
        close("z", ctx, fwd["z"].ref, fwd["z"].mag, z, tol=1e-14)
        close("d", ctx, fwd["d"].ref, fwd["d"].mag, d, tol=1e-14)
        bwd = MR.spatial_bwd(case.variant, t, dd, P, case.h, case.w, keep, case.p)
        assert set(bwd) == {"dt"} | {"g_" + k for k in MR.keys_of(case.variant)}, ctx
        for k, term in bwd.items():
            close(k, ctx, term.ref, term.mag, grads[k], tol=1e-14)
            assert bool((term.mag >= term.ref.abs() * (1 - 1e-12)).all()) and bool((term.a >= 0).all()) and bool((term.mf >= 0).all()), f"{k}: {ctx}"


def test_pre_restatement_agrees_with_autograd_through_layer_norm():
    for i, (M, D, mean) in enumerate([(1, 4, 0.0), (3, 64, 0.0), (5, 260, 0.0), (4, 772, 0.0), (37, 256, 1000.0)]):
        x, du, dy, nw, nb, gamma, gammax = MR.pre_operands(M, D, BF16, i, mean)
        xs, ws, bs, gs, gxs = (v.to(F64).clone().requires_grad_(True) for v in (x, nw, nb, gamma, gammax))
        u = F.layer_norm(xs, (D,), ws, bs, MR.EPS) * gs + xs * gxs
        u.backward(du.to(F64))
        ctx = f"M={M} D={D} mean={mean}"
        fwd = MR.pre_fwd(x, nw, nb, gamma, gammax)
        close("u", ctx, fwd["u"].ref, fwd["u"].mag, u.detach())
        bwd = MR.pre_bwd(du, x, dy, nw, nb, gamma, gammax)
        close("dx", ctx, bwd["dx"].ref, bwd["dx"].mag, xs.grad + dy.to(F64))
        for k, g in (("g_gamma", gs), ("g_gammax", gxs), ("g_nw", ws), ("g_nb", bs)):
            close(k, ctx, bwd[k].ref, bwd[k].mag, g.grad)
        assert "dx" not in MR.pre_bwd(du, x, None, nw, nb, gamma, gammax)


def test_kb_layout_is_the_row_major_tensor_permuted():
    for dt, g in ((BF16, 32), (F32, 16)):
        dx = torch.arange(5 * 4 * g, dtype=F32).reshape(5, 4 * g)
        kb = MR.kb_layout(dx, 8, dt)
        assert kb.shape == (4, 8, g) and bool(torch.isnan(kb[:, 5:]).all())
        for r in (0, 4):
            for c in (0, g - 1, g, 4 * g - 1):
                assert kb[c // g, r, c % g] == dx[r, c]


def test_gelu_terms_cover_the_fp32_emulation_of_gelu_parts():
    """The closed form without its two hardware terms against gelu_parts<false> emulated in fp32 with correctly rounded exp2 and reciprocal,
    over a dense grid; and the Lipschitz constants against the float64 functions."""
    z = torch.linspace(-12, 12, 2_400_001, dtype=F64).to(F32)
    g, dg = MR.gelu_parts_f32(z)
    z64 = z.to(F64)
    # x·Φ: |x|·ΔΦ and the product's rounding u·|gelu|;  gelu': the term itself
    err_g = (g.to(F64) - MR.gelu(z64)).abs()
    lim_g = z64.abs() * (MR.A_AS + MR.A_PHI_ROUND) + MR.U * MR.gelu(z64).abs()
    err_d = (dg.to(F64) - MR.dgelu(z64)).abs()
    assert float((err_g / lim_g.clamp_min(1e-300)).max()) <= 1.0, float((err_g / lim_g.clamp_min(1e-300)).max())
    assert float(err_d.max()) <= MR.A_AS + MR.A_DPHI_ROUND, float(err_d.max())
    print(f"gelu: worst error/limit {float((err_g / lim_g.clamp_min(1e-300)).max()):.3f}; gelu': {float(err_d.max()) / (MR.A_AS + MR.A_DPHI_ROUND):.3f}")
    zz = torch.linspace(-12, 12, 240_001, dtype=F64)
    assert MR.GP1 - 2e-6 <= float(MR.dgelu(zz).abs().max()) <= MR.GP1
    d2 = torch.exp(-0.5 * zz * zz) / math.sqrt(2 * math.pi) * (2 - zz * zz)
    assert MR.GP2 - 2e-6 <= float(d2.abs().max()) <= MR.GP2
    assert 3.4 < MR.DY < 3.5 and MR.A_AS < MR.A_PHI < 20 * MR.U and MR.A_PHI < MR.A_DPHI < 24 * MR.U


def test_launcher_formulas_and_tables():
    g = MR.limit_grids()
    # the issue's hand values
    assert g["bwd w=4 last fast"] == (50, 4) and g["bwd w=4 first per-pixel"] == (51, 4) and g["bwd w=4 last accepted"] == (52, 4) and g["bwd w=4 first refused"] == (53, 4)
    assert g["bwd w=14 last fast"] == (14, 14) and g["bwd w=14 first refused"] == (15, 14) and "bwd w=14 first per-pixel" not in g
    assert g["fwd w=14 last fast"] == (18, 14) and g["fwd w=14 first per-pixel"] == (19, 14) and g["fwd w=14 last accepted"] == (22, 14) and g["fwd w=14 first refused"] == (23, 14)
    assert g["fwd w=4 last fast"] == (66, 4) and g["fwd w=4 first per-pixel"] == (67, 4) and g["fwd w=4 last accepted"] == (78, 4) and g["fwd w=4 first refused"] == (79, 4)
    assert MR.accepted(14, 15, False) and not MR.accepted(14, 15, True)          # accepted forward, refused backward
    assert MR.accepted(13, 16, True) and not MR.accepted(19, 11, True)
    assert not MR.fast_path(F32, 5, 4, True) and not MR.fast_path(BF16, 4, 5, True)
    for case in MR.PIXEL_CASES:
        assert not MR.fast_path(case.dtype, case.h, case.w, True)
    for case in MR.FAST4_CASES + MR.FAST14_CASES:
        assert MR.fast_path(case.dtype, case.h, case.w, True) and MR.fast_path(case.dtype, case.h, case.w, False)
    for table in (MR.PIXEL_CASES, MR.FAST4_CASES, MR.FAST14_CASES):
        for dt in {c.dtype for c in table}:
            for v in MR.VARIANTS:
                assert {c.p for c in table if c.variant == v and c.dtype == dt} == {0.0, 0.1, 0.5}
        for grid in {(c.h, c.w) for c in table}:
            assert any(c.kind == "Z" for c in table if (c.h, c.w) == grid)       # stencil visibility: a zero projector at every grid


def test_conditions_on_the_inputs():
    """Decided by the reference alone, over every case of every table: hidden pre-activations away from zero with both signs present, mixing
    weights inside [0.1, 0.8], |z| ≤ 8, the kept fraction within 5σ of 1 − p."""
    seen = set()
    for case in MR.all_spatial_cases():
        if case in seen:
            continue
        seen.add(case)
        ctx = MR.case_name(case)
        t, dd, P, keep = MR.case_inputs(case)
        st = MR._forward(case.variant, t.to(F64), P, case.h, case.w)
        assert float(st["z"].abs().max()) <= 8.0, f"{ctx}: |z| {float(st['z'].abs().max())}"
        if MR.has_noise(case.variant):
            hp = st["hpre"]
            assert float(hp.abs().min()) >= 0.05 and bool((hp > 0).any()) and bool((hp < 0).any()), f"{ctx}: hpre {float(hp.abs().min())}"
            assert float(st["wts"].min()) >= 0.1 and float(st["wts"].max()) <= 0.8, f"{ctx}: weights {st['wts'].min()} .. {st['wts'].max()}"
        if keep is not None:
            n = keep.numel()
            assert abs(float(keep.float().mean()) - (1 - case.p)) <= 5 * math.sqrt(case.p * (1 - case.p) / n), f"{ctx}: kept {float(keep.float().mean())}"
        else:
            assert case.p == 0.0
    for kind in "AZ":
        for v in MR.VARIANTS:
            P = MR.spatial_params(v, kind)
            assert set(P) == set(MR.keys_of(v)) and (kind == "A" or (not P["proj_w"].any() and not P["proj_b"].any()))


# ------------------------------------------------------------------------------------------ planted bugs
BUG_CASES = [Case(F32, "hybrid", "Z", 2, 1, 1, 0.0, None), Case(F32, "hybrid", "Z", 2, 2, 3, *MR.DROPS[1]), Case(F32, "hybrid", "Z", 2, 3, 7, 0.0, None),
             Case(F32, "hybrid", "A", 2, 5, 4, *MR.DROPS[1]), Case(F32, "noise_aware", "A", 2, 1, 4, 0.0, None), Case(F32, "hybrid", "Z", 2, 9, 9, 0.0, None)]
SPATIAL_BUGS = {"border_tap": "one border tap not zeroed (reads token 0)", "hw_swapped": "h and w swapped on a non-square grid",
                "last_pixel": "the last pixel of the last pixel group skipped", "cls_through": "the CLS row sent through the operator",
                "identity_filtered": "the identity taken from the filtered input", "weights_exchanged": "two mixing weights exchanged",
                "last_image": "the last image left out of a parameter gradient", "pool_gradient": "the pool gradient dpool/hw dropped from dt",
                "relu_gate": "the ReLU gate ignored"}


def margin(good, bad, cnt, count_of):
    """Worst |bad − good| / bound over every output, under the fp32 bound and under the fast kernel's bound (bf16 storage, the MFMA term)."""
    out = []
    for dt, fast in ((F32, False), (BF16, True)):
        worst = 0.0
        for k, term in good.items():
            stored = dt if k in ("d", "dt", "u", "dxT") else F32
            b = MR.bound(term, count_of(cnt, k), stored, fast)
            worst = max(worst, float(((bad[k].ref - term.ref).abs() / b.clamp_min(1e-300)).max()))
        out.append(worst)
    return out


def test_planted_spatial_bugs_exceed_the_bounds():
    report = []
    for bug, what in SPATIAL_BUGS.items():
        best = [0.0, 0.0]
        for case in BUG_CASES:
            t, dd, P, keep = MR.case_inputs(case)
            good = MR.spatial_bwd(case.variant, t, dd, P, case.h, case.w, keep, case.p)
            bad = MR.spatial_bwd(case.variant, t, dd, P, case.h, case.w, keep, case.p, bug=bug)
            good["d"] = MR.spatial_fwd(case.variant, t, P, case.h, case.w, keep, case.p)["d"]
            bad["d"] = MR.spatial_fwd(case.variant, t, P, case.h, case.w, keep, case.p, bug=bug)["d"]
            best = [max(a, b) for a, b in zip(best, margin(good, bad, None, lambda _, k: 1))]
        report.append(f"{what}: {best[0]:.3g}x the fp32 bound, {best[1]:.3g}x the fast kernel's bound")
    print("\n".join(report))
    assert all(float(r.split(": ")[1].split("x")[0]) >= 10 and float(r.split(", ")[1].split("x")[0]) >= 10 for r in report), "\n".join(report)


def test_planted_pre_bugs_exceed_the_bounds():
    report = []
    for bug, what in (("dgamma_s1", "dγ built from S1 alone"), ("odd_wave_row", "the last row of an odd-count wave dropped from the column sums")):
        best = [0.0, 0.0]
        for i, (M, D) in enumerate(((5, 64), (3, 260), (8197, 64))):
            x, du, dy, nw, nb, gamma, gammax = MR.pre_operands(M, D, BF16, i)
            good = MR.pre_bwd(du, x, dy, nw, nb, gamma, gammax)
            bad = MR.pre_bwd(du, x, dy, nw, nb, gamma, gammax, bug=bug)
            best = [max(a, b) for a, b in zip(best, margin(good, bad, M, lambda m, k: MR.pre_count(k, m)))]
        report.append(f"{what}: {best[0]:.3g}x, {best[1]:.3g}x")
        assert min(best) >= 10, report[-1]
    # the K-blocked copy: judged as the T copy of dx (its own rounding alone, since it must equal the row-major copy bit for bit)
    x, du, dy, nw, nb, gamma, gammax = MR.pre_operands(5, 256, BF16, 9)
    dx = MR.pre_bwd(du, x, dy, nw, nb, gamma, gammax)["dx"]
    good, bad = MR.kb_layout(dx.ref, 5, BF16), MR.kb_layout(dx.ref, 5, BF16, bug="kb_offset")
    ratio = float(((bad - good).abs() / (MR.kb_layout(MR.bound(dx, MR.C_DX, BF16), 5, BF16))).max())
    report.append(f"a K-blocked column block offset by one: {ratio:.3g}x")
    print("\n".join(report))
    assert ratio >= 10, report[-1]
