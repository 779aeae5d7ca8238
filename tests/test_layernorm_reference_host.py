"""CPU: the yardstick of tests/test_layernorm_contract_gpu.py.  Every restatement of tests/layernorm_reference.py against a second form (float64 autograd
through torch.nn.functional.layer_norm); the three-byte codec over a sweep of bit patterns (bit for bit against uia_hip.ops, its three error figures,
the overflow condition, sign symmetry and monotonicity, the K-blocked layout); an fp32 emulation of the kernels' order of operations judged by the
bounds over the whole case tables (every ratio ≤ 1: the derivation has missed no rounding); planted bugs in that emulation, each of which must exceed a
bound somewhere; and every refusal of the launchers, which return before the first HIP call."""
import torch
import torch.nn.functional as F

import helpers_reference as R
import layernorm_reference as LR

F64, F32, BF16, I8 = LR.F64, LR.F32, LR.BF16, LR.I8


# ------------------------------------------------------------------------------------------ second forms
def test_restatements_agree_with_autograd_through_layer_norm():
    for case in LR.bwd_cases()[::3] + LR.bwd_cases()[1::7]:
        dy, x, gamma, dres = LR.bwd_inputs(case)
        beta = LR.affine(case.D, 5)[1]
        eps = LR.eps32(case.eps)
        x64 = x.to(F64).requires_grad_(True)
        y = F.layer_norm(x64, (case.D,), gamma.to(F64), beta.to(F64), eps)
        fwd = LR.ln_fwd(x, gamma, beta, case.eps)
        scale = lambda t: float(t.abs().max()) + 1e-300                                                                  # noqa: E731
        assert float((fwd["y"].ref - y.detach()).abs().max()) <= 1e-12 * scale(y.detach()), case
        mu = x.to(F64).mean(1)
        var = x.to(F64).var(1, unbiased=False)
        assert torch.allclose(fwd["mean"].ref, mu, rtol=1e-13, atol=0) and torch.allclose(fwd["rstd"].ref, (var + eps).rsqrt(), rtol=1e-12, atol=0)
        tot = (y * dy.to(F64)).sum() + (0 if dres is None else (x64 * dres.to(F64)).sum())            # d/dx adds dres
        tot.backward()
        got = LR.ln_bwd(dy, x, gamma, case.eps, dres)
        # the constant rows at eps = 1e-12 are ill conditioned even in float64 (rstd = 1e6 on cancellation noise of 1e-16·|c|): judge against the terms' size
        assert float(((got.ref - x64.grad).abs() / (got.mag + 1e-300)).max()) <= 1e-11, case
        assert bool((got.mag >= got.ref.abs() * (1 - 1e-12)).all()) and bool((fwd["y"].mag >= fwd["y"].ref.abs() * (1 - 1e-12)).all())


def test_periodic_restatement_is_the_dense_one_on_zero_padded_rows():
    for case in LR.periodic_cases():
        dy, x, gamma, dres_rows, _ = LR.periodic_inputs(case)
        dense = torch.zeros(case.M, case.D)
        dense[0::case.period] = dres_rows
        a, b = LR.ln_bwd_periodic(dy, x, gamma, case.eps, dres_rows, case.period), LR.ln_bwd(dy, x, gamma, case.eps, dense)
        assert torch.equal(a.ref, b.ref) and torch.equal(a.mag, b.mag), case


def test_pool_restatement_is_layer_norm_then_mean():
    for case in LR.pool_cases():
        x, gamma, beta = LR.pool_inputs(case)
        y = F.layer_norm(x.to(F64), (case.D,), gamma.to(F64), beta.to(F64), LR.eps32(case.eps))[:, case.row0:case.row0 + case.n].mean(1)
        got = LR.ln_mean_rows(x, gamma, beta, case.eps, case.row0, case.n)
        assert float(((got.ref - y).abs() / got.mag.clamp_min(1e-300)).max()) <= 1e-11, case


# ------------------------------------------------------------------------------------------ the codec
def test_codec_over_the_bit_pattern_sweep():
    from uia_hip import ops
    bits = LR.sweep_bits()
    assert bits.numel() == 65536 * 19
    x = LR.float_of(bits)
    ok = ~torch.isnan(x)
    x = x[ok]
    hi, lo = LR.encode3(x)
    ohi, olo = ops.float_to_three_byte(x)
    assert torch.equal(hi.view(torch.int16), ohi.view(torch.int16)) and torch.equal(lo, olo)
    assert torch.equal(hi.view(torch.int16), x.bfloat16().view(torch.int16))
    dec = LR.decode3(hi, lo)
    assert torch.equal(LR.bits_of(dec), LR.bits_of(ops.three_byte_to_float(hi[None], lo[None])[0]))
    assert int(lo.min()) == -127 and int(lo.max()) == 127

    mag_bits = LR.bits_of(x) & 0x7FFFFFFF
    finite = mag_bits < 0x7F800000
    # overflow: the hi plane is inf from THREE_MAX_BITS on, the decoded value from THREE_INF_BITS on, and neither below
    hi_inf = torch.isinf(hi.float())
    assert torch.equal(hi_inf & finite, (mag_bits >= LR.THREE_MAX_BITS) & finite)
    assert torch.equal(torch.isinf(dec) & finite, (mag_bits >= LR.THREE_INF_BITS) & finite)
    assert 0x7F7FFF7F < LR.THREE_INF_BITS and bool(torch.isfinite(LR.decode3(*LR.encode3(LR.float_of(torch.tensor([0x7F7FFF7F, 0xFF7FFF7F]))))).all())

    inside = mag_bits < LR.THREE_MAX_BITS
    xi, di, li = x[inside].to(F64), dec[inside].to(F64), lo[inside]
    # which elements the clamp touched, from the bit arithmetic of the docstring
    L = LR.bits_of(x[inside]) & 0xFFFF
    hs = LR.hi_bits(hi[inside])
    up = hs != ((LR.bits_of(x[inside]) >> 16) & 0xFFFF)
    clamped = (~up & (L >= 0x7F80) & (L <= 0x8000)) | (up & (L >= 0x8000) & (L <= 0x807F))
    d_raw = ((LR.bits_of(x[inside]) + 0x80) >> 8) - (hs << 8)
    assert int(d_raw.min()) == -128 and int(d_raw.max()) == 128 and torch.equal(clamped, d_raw.abs() == 128) and torch.equal(li.to(torch.int64), d_raw.clamp(-127, 127))
    normal = xi.abs() >= 2.0 ** -126
    err = (di - xi).abs()
    rel = err[normal] / xi[normal].abs()
    assert float(rel[~clamped[normal]].max()) <= LR.U3_UNCLAMPED
    worst = float(rel[clamped[normal]].max())
    assert worst <= LR.U3 and abs(worst / 2.0 ** -16 - 2 / (1 + 2.0 ** -8)) < 1e-12                  # 1.992·2^-16, at L = 0x8000 on an even hi with a zero mantissa
    assert float(err[~normal].max()) <= LR.A3 and float(err[~normal].max()) == LR.A3              # subnormals: 256 steps of 2^-149, reached
    # what bound() allows a three-byte result covers all of it
    assert bool((err <= LR.U3 * xi.abs() + LR.A3).all())

    # odd symmetry and monotonicity of decode∘encode on the finite inputs inside the condition
    pos = LR.float_of(bits[(bits < LR.THREE_MAX_BITS)])
    dpos = LR.decode3(*LR.encode3(pos))
    dneg = LR.decode3(*LR.encode3(-pos))
    assert torch.equal(LR.bits_of(dneg), LR.bits_of(-dpos))
    assert bool((pos[1:] > pos[:-1]).all()) and bool((dpos[1:] >= dpos[:-1]).all())
    # the values the GPU test sends through the device encoder obey the condition, and the planes it sends through the decoder are finite
    LR.check_three(LR.sweep_values())
    shi, slo = LR.sweep_planes()
    sdec = LR.decode3(shi, slo)
    assert bool(torch.isfinite(sdec).all()) and not bool(((sdec == 0) & torch.signbit(sdec)).any()) and {int(v) for v in slo.unique()} == set(LR.LOW_BYTES)


def test_k_blocked_layout_round_trip_with_more_rows_than_m():
    M, D, total = 5, 96, 9
    hi = LR.rnd(M, D, seed=1).bfloat16()
    kb = LR.kblock(hi, total)
    assert kb.shape == (3, total, 32) and bool(torch.isnan(kb[:, M:].float()).all())
    assert torch.equal(LR.unkblock(kb, M).view(torch.int16), hi.view(torch.int16))
    assert torch.equal(kb[2, 3].view(torch.int16), hi[3, 64:96].view(torch.int16))
    assert not torch.equal(LR.unkblock(kb, M, rows_in_address=M).view(torch.int16), hi.view(torch.int16))
    assert torch.equal(LR.unkblock(LR.kblock(hi, M), M).view(torch.int16), hi.view(torch.int16))


# ------------------------------------------------------------------------------------------ the fp32 emulation
def f32(v):
    return torch.tensor(v, dtype=F32)


def fma(a, b, c):
    """One rounding: a·b is exact in float64, and the double rounding of the sum is below 2^-29 relative."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def lanes(x, nv):
    """[M, D] -> [M, nv, 64, 4]: float4 c = lane + 64·k of the row, zero beyond D (a row wider than nv·256 loses its tail: the planted NV bug)."""
    M, D = x.shape
    p = torch.zeros(M, max(D, nv * 256), dtype=F32)
    p[:, :D] = x
    return p[:, :nv * 256].reshape(M, nv, 64, 4)


def unlanes(v, D):
    M = v.shape[0]
    out = v.reshape(M, -1)
    if out.shape[1] < D:                      # the elements the planted NV bug never wrote
        out = torch.cat([out, torch.full((M, D - out.shape[1]), float("nan"))], 1)
    return out[:, :D]


def valid(D, nv):
    return (torch.arange(nv * 256) < D).reshape(1, nv, 64, 4)


def wave_sum(s):
    """uia_common.h wave_sum: quad partners at distance 1 and 2, the other quad, the other half-row, the other row, the other half-wave — a balanced
    tree over the lanes in index order (fp32 addition commutes, so every lane holds the same bits)."""
    for _ in range(6):
        s = s[:, 0::2] + s[:, 1::2]
    return s


def emu_stats(x, eps, nv, bug=None):
    """mean [M, 1], rstd [M, 1] and d = x − mean in lane layout (zero beyond D), as ln_fwd_kernel / ln_bwd_kernel / ln_mean_partial_kernel."""
    M, D = x.shape
    v, ok = lanes(x, nv), valid(D, nv)
    s = torch.zeros(M, 64)
    for k in range(nv):
        s = s + (((v[:, k, :, 0] + v[:, k, :, 1]) + v[:, k, :, 2]) + v[:, k, :, 3])
    mean = (wave_sum(s) / f32(nv * 256 if bug == "mean_padded" else D)).reshape(M, 1, 1, 1)
    q = torch.zeros(M, 64)
    if bug == "single_pass":
        for k in range(nv):
            for e in range(4):
                q = fma(v[:, k, :, e], v[:, k, :, e], q)
        var = wave_sum(q) / f32(D) - mean.reshape(M, 1) * mean.reshape(M, 1)
        d = torch.where(ok, v - mean, torch.zeros(()))
    else:
        d = torch.where(ok, v - mean, torch.zeros(()))
        for k in range(nv):
            for e in range(4):
                q = fma(d[:, k, :, e], d[:, k, :, e], q)
        var = wave_sum(q) / f32({"var_padded": nv * 256, "var_d_minus_1": D - 1}.get(bug, D))
    e32 = f32(eps)
    if bug == "eps_dropped":
        rstd = (1 / var.to(F64).sqrt()).to(F32)
    elif bug == "eps_after_sqrt":
        rstd = (1 / (var.to(F64).sqrt().to(F32) + e32).to(F64)).to(F32)
    else:
        rstd = (1 / (var + e32).to(F64).sqrt()).to(F32)                 # a correctly rounded rsqrt
    return mean, rstd.reshape(M, 1, 1, 1), d


def emu_fwd(x, gamma, beta, eps, bug=None):
    """y32 [M, D], mean [M], rstd [M] of ln_fwd_kernel."""
    M, D = x.shape
    nv = 3 if bug == "nv3" else LR.NV_FWD
    mean, rstd, _ = emu_stats(x, eps, nv, bug)
    v = lanes(x, nv)
    if bug == "gamma_shifted":
        gamma = gamma.roll(-4)
    g, b = lanes(gamma[None], nv), lanes(beta[None], nv)
    y = fma((v - mean) * rstd, g, b)
    return unlanes(y, D), mean.reshape(M), rstd.reshape(M)


def emu_bwd(dy, x, gamma, eps, dres=None, bug=None, period=None, dres_rows=None):
    """dx (fp32, before it is stored) of ln_bwd_kernel: dy holds the storage type's values; x and dres what the kernel has decoded."""
    M, D = x.shape
    nv = 3 if bug == "nv3" else LR.nv_bwd(D)
    if bug == "gamma_shifted":
        gamma = gamma.roll(-4)
    g = lanes(dy, nv) * lanes(gamma[None], nv)
    mean, rstd, d = emu_stats(x, eps, nv, bug)
    xh = d * rstd
    sg, sgx = torch.zeros(M, 64), torch.zeros(M, 64)
    for k in range(nv):
        for e in range(4):
            sg = sg + g[:, k, :, e]
            sgx = fma(g[:, k, :, e], xh[:, k, :, e], sgx)
    mg = (wave_sum(sg) / f32(D // 4 if bug == "mean_g_quarter" else D)).reshape(M, 1, 1, 1)
    mgx = (wave_sum(sgx) / f32(D // 4 if bug == "mean_gx_quarter" else D)).reshape(M, 1, 1, 1)
    o = torch.zeros(M, nv, 64, 4)
    if period is not None:
        dense = torch.zeros(M, D)
        r = torch.arange(M)
        if bug == "div_mod_swapped":
            has, src = r // period == 0, r % period
        elif bug == "every_row_residual":
            has, src = torch.ones(M, dtype=torch.bool), r // period
        else:
            has, src = r % period == 0, r // period
        src = src.clamp_max(dres_rows.shape[0] - 1)
        dense[has] = dres_rows[src[has]]
        o = lanes(dense, nv)
    elif dres is not None and bug != "dres_omitted":
        o = lanes(dres, nv)
        if bug == "dres_twice":
            o = o + o
    t = (g - mg) + xh * mgx if bug == "xhat_sign" else (g - mg) - xh * mgx
    return unlanes(o + rstd * t, D)


def emu_pool(x, gamma, beta, eps, row0, n, bug=None):
    """out [B, D] of ln_mean_partial_kernel + ln_mean_final_kernel: slices of per rows, a wave's rows 4 apart, waves then slices in order."""
    B, L, D = x.shape
    rows_ = x[:, row0:row0 + n].reshape(B * n, D)
    mean, rstd, _ = emu_stats(rows_, eps, LR.NV_FWD, bug)
    xh = unlanes((lanes(rows_, LR.NV_FWD) - mean) * rstd, D).reshape(B, n, D)
    per = -(-n // LR.POOL_SLICES)
    total = torch.zeros(B, D)
    for sl in range(LR.POOL_SLICES):
        lo, hi = sl * per, min(sl * per + per, n)
        acc = [torch.zeros(B, D) for _ in range(4)]
        if not (bug == "short_slice_dropped" and lo < n and hi - lo < per):
            for w in range(4):
                for r in range(lo + w, hi, 4):
                    acc[w] = acc[w] + xh[:, r]
        total = total + (((acc[0] + acc[1]) + acc[2]) + acc[3])
    inv = f32(1.0) / f32(per * LR.POOL_SLICES if bug == "pool_per_32" else n)
    return fma(total * inv, gamma[None], beta[None])


def three_decoded(case, planes, bug=None):
    """x and dres as an emulated kernel reads them from the planes (K-blocked where the case says so)."""
    out = {}
    for name, form in (("x", case.x if hasattr(case, "x") else "kb"), ("dres", getattr(case, "dres", "none"))):
        if name + "_hi" not in planes:
            continue
        hi = planes[name + "_hi"]
        M, D = hi.shape
        if form == "kb" and D % 32 == 0:
            kb = LR.kblock(hi, M + case.kb_extra, fill=0.0)
            hi = LR.unkblock(kb, M, rows_in_address=M if bug == "kb_rows_is_m" else None)
        out[name] = LR.decode3(hi, planes[name + "_lo"], bug=bug if bug == "zero_extended" else None)
    return out


class Ratios:
    """Worst error/bound per bar."""

    def __init__(self):
        self.ck = R.Checker()

    def add(self, bar, got, term, out, ctx):
        return self.ck.check(bar, got, term.ref, LR.bound(term, out), ctx)

    def worst(self):
        return {k: v[0] for k, v in self.ck.worst.items()}


def store(v, dt):
    return v.to(dt).to(F32)


def run_tables(bug=None, only=None):
    """The emulation with `bug` planted over every case table, judged like the GPU test judges the kernels: Ratios."""
    rt = Ratios()
    codec_bug = bug if bug in ("hi_truncated", "no_clamp") else None
    if only in (None, "fwd"):
        for case in LR.fwd_cases():
            if bug == "nv3" and case.D != 772:
                continue
            x, gamma, beta = LR.fwd_inputs(case)
            ref = LR.ln_fwd(x, gamma, beta, case.eps)
            y, mean, rstd = emu_fwd(x, gamma, beta, case.eps, bug)
            ctx = LR.name_of(case)
            rt.add("fwd y fp32", y, ref["y"], F32, ctx)
            rt.add("fwd y bf16", store(y, BF16), ref["y"], BF16, ctx)
            rt.add("fwd mean", mean, ref["mean"], F32, ctx)
            rt.add("fwd rstd", rstd, ref["rstd"], F32, ctx)
    if only in (None, "bwd"):
        for case in LR.bwd_cases():
            if bug == "nv3" and case.D != 772:
                continue
            dy, x, gamma, dres = LR.bwd_inputs(case)
            ref = LR.ln_bwd(dy, x, gamma, case.eps, dres)
            o = emu_bwd(dy, x, gamma, case.eps, dres, bug)
            rt.add("bwd dx fp32", o, ref, F32, LR.name_of(case))
            rt.add("bwd dx bf16", store(o, BF16), ref, BF16, LR.name_of(case))
    if only in (None, "three"):
        for case in LR.three_cases():
            if bug == "nv3" and case.D != 772:
                continue
            dy, x, gamma, dres, planes = LR.three_inputs(case)
            ref = LR.ln_bwd(dy, x, gamma, case.eps, dres)
            seen = three_decoded(case, planes, bug)
            o = emu_bwd(dy, seen.get("x", x), gamma, case.eps, seen.get("dres", dres), bug)
            ctx = LR.name_of(case)
            if "dx32" in case.outs:
                rt.add("three dx32", o, ref, F32, ctx)
            if "dx_lo" in case.outs:
                if bool(torch.isfinite(o).all()):
                    hi, lo = LR.encode3(o, bug=codec_bug)
                    rt.add("three decoded", LR.decode3(hi, lo, bug=bug if bug == "zero_extended" else None), ref, LR.THREE, ctx)
                    rt.add("three hi plane", hi.float(), ref, BF16, ctx)
                else:
                    rt.add("three decoded", o, ref, LR.THREE, ctx)
            else:
                rt.add("three dxT", store(o, BF16), ref, BF16, ctx)
    if only in (None, "periodic"):
        for case in LR.periodic_cases():
            if bug == "nv3" and case.D != 772:
                continue
            dy, x, gamma, dres_rows, planes = LR.periodic_inputs(case)
            ref = LR.ln_bwd_periodic(dy, x, gamma, case.eps, dres_rows, case.period)
            seen = three_decoded(case, planes, bug)
            o = emu_bwd(dy, seen.get("x", x), gamma, case.eps, None, bug, period=case.period, dres_rows=dres_rows)
            ctx = LR.name_of(case)
            if case.form == "f32":
                rt.add("periodic fp32", o, ref, F32, ctx)
            elif bool(torch.isfinite(o).all()):
                hi, lo = LR.encode3(o, bug=codec_bug)
                rt.add("periodic three-byte", LR.decode3(hi, lo, bug=bug if bug == "zero_extended" else None), ref, LR.THREE, ctx)
            else:
                rt.add("periodic three-byte", o, ref, LR.THREE, ctx)
    if only in (None, "pool"):
        for case in LR.pool_cases():
            x, gamma, beta = LR.pool_inputs(case)
            ref = LR.ln_mean_rows(x, gamma, beta, case.eps, case.row0, case.n)
            rt.add("pool", emu_pool(x, gamma, beta, case.eps, case.row0, case.n, bug), ref, F32, LR.name_of(case))
    return rt


def test_case_tables_cover_the_issue_and_obey_the_input_conditions():
    fwd, bwd, three, per, pool = LR.fwd_cases(), LR.bwd_cases(), LR.three_cases(), LR.periodic_cases(), LR.pool_cases()
    for dt in LR.DTYPES:
        f = [c for c in fwd if c.dtype == dt]
        b = [c for c in bwd if c.dtype == dt]
        assert {c.D for c in f} == set(LR.WIDTHS) == {c.D for c in b}
        assert {c.M for c in f} == set(LR.ROWS) == {c.M for c in b}
        assert {c.eps for c in f} == set(LR.EPSS) == {c.eps for c in b}
        assert {c.outs for c in f} == set(LR.FWD_OUTS) and {c.ld for c in f} == set(LR.FWD_LD)
        assert {(c.outs, c.dres) for c in b} == {(o, d) for o in LR.BWD_OUTS for d in (False, True)} and {(c.ld, c.dres) for c in b} == {(ld, d) for ld in LR.BWD_LD for d in (False, True)}
    assert [LR.nv_bwd(D) for D in LR.WIDTHS] == [3, 3, 3, 3, 3, 3, 4, 4]
    assert {c.D for c in three if "kb" not in (c.x, c.dres)} == set(LR.THREE_D) and {c.D for c in three if "kb" in (c.x, c.dres)} == set(LR.THREE_D_KB)
    assert {c.x for c in three} == {"f32", "rm", "kb"} and {c.dres for c in three} == {"none", "f32", "rm", "kb"} and {c.outs for c in three} == set(LR.THREE_OUTS)
    assert {c.kb_extra for c in three if "kb" in (c.x, c.dres)} == {0, 3} and {c.M for c in three} == set(LR.ROWS)
    assert all(c.x != "f32" or c.dres in ("rm", "kb") or "dx_lo" in c.outs for c in three)
    assert {(c.M, c.period) for c in per} == {(M, p) for M in LR.PERIODIC_M for p in (1, 2, 5, M, M + 1)} and {c.form for c in per} == set(LR.PERIODIC_FORMS)
    assert any(c.form == "bf16x3" and c.D % 32 == 0 and c.kb_extra for c in per) and any(c.form == "bf16x3" and c.D % 32 for c in per)
    assert {c.n for c in pool} == set(LR.POOL_N) and {c.B for c in pool} == set(LR.POOL_B) and {c.D for c in pool} == set(LR.POOL_D)
    assert all({c.row0 for c in pool if c.n == n} == {0, 1, 2} and all(c.row0 + c.n <= c.L for c in pool) for n in LR.POOL_N)
    assert 30 <= len(fwd) <= 40 and 30 <= len(bwd) <= 40
    for case in fwd:
        x, gamma, beta = LR.fwd_inputs(case)
        LR.check_conditions(x)
        assert bool((gamma == 0).any()) and bool((gamma < 0).any()) and bool((beta == 0).any()) and bool((beta < 0).any())
    for case in bwd:
        LR.check_conditions(LR.bwd_inputs(case)[1])
    for case in three:
        dy, x, gamma, dres, planes = LR.three_inputs(case)
        LR.check_conditions(x)
        for t in (x, dres):
            if t is not None:
                LR.check_three(t)
    for case in per:
        LR.check_conditions(LR.periodic_inputs(case)[1])
    for case in pool:
        LR.check_conditions(LR.pool_inputs(case)[0])
    kinds = {LR.KINDS[(i + c.first) % 6] for c in fwd for i in range(c.M)}
    assert kinds == set(LR.KINDS)


def test_the_fp32_emulation_stays_inside_every_bound():
    rt = run_tables()
    print(rt.ck.report())
    assert rt.ck.ok(), rt.ck.report()
    assert set(rt.worst()) == {"fwd y fp32", "fwd y bf16", "fwd mean", "fwd rstd", "bwd dx fp32", "bwd dx bf16", "three dx32", "three decoded", "three hi plane",
                               "three dxT", "periodic fp32", "periodic three-byte", "pool"}
    assert all(0 < v <= 1.0 for v in rt.worst().values())


# bug -> (table it is planted in, bars of which one must fail)
PLANTED = {
    "mean_padded": "fwd", "var_padded": "fwd", "single_pass": "fwd", "eps_dropped": "fwd", "eps_after_sqrt": "fwd", "var_d_minus_1": "fwd", "nv3": "bwd",
    "gamma_shifted": "fwd", "dres_omitted": "bwd", "dres_twice": "bwd", "mean_g_quarter": "bwd", "mean_gx_quarter": "bwd", "xhat_sign": "bwd",
    "div_mod_swapped": "periodic", "every_row_residual": "periodic", "kb_rows_is_m": "three", "zero_extended": "three", "no_clamp": "three",
    "hi_truncated": "three", "pool_per_32": "pool", "short_slice_dropped": "pool",
}


def test_every_planted_bug_exceeds_a_bound():
    lines = []
    for bug, table in PLANTED.items():
        rt = run_tables(bug, only=table)
        worst = max(rt.worst().values())
        lines.append(f"{bug}: {worst:.3g} ({max(rt.worst(), key=rt.worst().get)})")
        assert not rt.ck.ok() and worst > 1.0, (bug, rt.worst())
    print("\n".join(lines))
    # the same bugs in the backward's statistics (the kernel repeats them) and the NV bug in the forward's table run the same code
    for bug, table in (("mean_padded", "bwd"), ("single_pass", "bwd"), ("var_d_minus_1", "three"), ("gamma_shifted", "bwd"), ("eps_dropped", "pool")):
        assert not run_tables(bug, only=table).ck.ok(), (bug, table)


def test_no_clamp_bug_is_caught_at_the_codec_alone():
    """The clamp matters on 1/256 of all values, so a table of random rows may hold none: the sweep holds every one."""
    x = LR.sweep_values()
    hi, lo = LR.encode3(x, bug="no_clamp")
    err = (LR.decode3(hi, lo).to(F64) - x.to(F64)).abs()
    assert not bool((err <= LR.U3 * x.to(F64).abs() + LR.A3).all())
    for bug in ("hi_truncated",):
        hi, lo = LR.encode3(x, bug=bug)
        assert not bool(((LR.decode3(hi, lo).to(F64) - x.to(F64)).abs() <= LR.U3 * x.to(F64).abs() + LR.A3).all())
    hi, lo = LR.encode3(x)
    assert not bool(((LR.decode3(hi, lo, bug="zero_extended").to(F64) - x.to(F64)).abs() <= LR.U3 * x.to(F64).abs() + LR.A3).all())


# ------------------------------------------------------------------------------------------ refusals
X, G, B_, DY, O1, O2, ST, HI, LO, HI2, LO2, OLO, WS = (0x100000 * k for k in range(1, 14))          # addresses that are never followed


def test_every_refusal_comes_before_anything_is_enqueued():
    from uia_hip import _lib
    lib = _lib.lib()
    BF, FP = _lib.BF16, _lib.F32

    def refused(rc, word, name):
        err = lib.uia_last_error().decode()
        assert rc != 0 and word in err and name in err, (rc, err, word)

    def fwd(dt=FP, M=4, D=64, ld=64, x=X, g=G, b=B_, eps=1e-5, yT=O1, y32=O2, st=ST):
        return lib.uia_layernorm_fwd_stats(None, dt, M, D, ld, x, g, b, eps, yT, y32, st)

    for D in (0, 6, 1028):
        refused(fwd(D=D, ld=1028), "unsupported shape", "uia_layernorm_fwd")
    refused(fwd(M=0), "unsupported shape", "uia_layernorm_fwd")
    refused(fwd(ld=60), "row stride", "uia_layernorm_fwd")
    refused(fwd(ld=66), "row stride", "uia_layernorm_fwd")
    refused(fwd(yT=None, y32=None, st=None), "null tensor", "uia_layernorm_fwd")
    refused(lib.uia_layernorm_fwd(None, FP, 4, 64, 64, X, G, B_, 1e-5, None, None), "null tensor", "uia_layernorm_fwd")
    refused(fwd(x=None), "null tensor", "uia_layernorm_fwd")
    refused(fwd(x=X + 4), "alignment", "uia_layernorm_fwd")
    refused(fwd(st=ST + 4), "alignment", "uia_layernorm_fwd")
    refused(fwd(dt=7), "bad dtype", "uia_layernorm_fwd")

    def bwd3(dt=BF, M=4, D=64, ld=64, dy=DY, x=X, x_hi=None, x_lo=None, x_kb=0, g=G, eps=1e-5, dres=None, r_hi=None, r_lo=None, r_kb=0, dx32=O1, dxT=O2, dx_lo=None):
        return lib.uia_layernorm_bwd3(None, dt, M, D, ld, dy, x, x_hi, x_lo, x_kb, g, eps, dres, r_hi, r_lo, r_kb, dx32, dxT, dx_lo)

    name = "uia_layernorm_bwd"
    for D in (0, 6, 1028):
        refused(bwd3(D=D, ld=1028), "unsupported shape", name)
        refused(lib.uia_layernorm_bwd(None, FP, 4, D, 1028, DY, X, G, 1e-5, None, O1, None), "unsupported shape", name)
    refused(bwd3(ld=60), "row stride", name)
    refused(bwd3(ld=66), "row stride", name)
    refused(bwd3(dx32=None, dxT=None), "null tensor", name)
    refused(bwd3(x=None), "null tensor", name)
    refused(bwd3(dt=FP, dx_lo=OLO), "three-byte tensors need bf16", name)
    refused(bwd3(ld=68, dx_lo=OLO), "compact rows", name)
    refused(bwd3(x_hi=HI, x_lo=LO), "x as a three-byte tensor", name)                          # x given together with x_lo
    refused(bwd3(x=None, x_lo=LO), "null tensor", name)                                        # x_lo without x_hi
    refused(bwd3(x_lo=LO), "x as a three-byte tensor", name)                                   # x_lo without x_hi, beside an fp32 x
    refused(bwd3(x=None, x_hi=HI, x_lo=LO, x_kb=3), "x as a three-byte tensor", name)          # x_kb_rows < M
    refused(bwd3(D=48, ld=48, x=None, x_hi=HI, x_lo=LO, x_kb=4), "x as a three-byte tensor", name)   # D % 32
    refused(bwd3(x_kb=4), "x_kb_rows without a three-byte x", name)
    refused(bwd3(x=None, x_hi=HI + 4, x_lo=LO), "x as a three-byte tensor", name)              # odd plane alignments
    refused(bwd3(x=None, x_hi=HI, x_lo=LO + 2), "x as a three-byte tensor", name)
    refused(bwd3(dres=O1 + 64, r_hi=HI2, r_lo=LO2), "dres as a three-byte tensor", name)       # dres given together with dres_lo
    refused(bwd3(r_lo=LO2), "dres as a three-byte tensor", name)                               # dres_lo without dres_hi
    refused(bwd3(r_hi=HI2 + 2, r_lo=LO2), "dres as a three-byte tensor", name)
    refused(bwd3(r_hi=HI2, r_lo=LO2 + 1), "dres as a three-byte tensor", name)
    refused(bwd3(r_kb=4, dx_lo=OLO), "dres_kb_rows needs a three-byte dres", name)             # dres_kb_rows without dres_lo
    refused(bwd3(r_hi=HI2, r_lo=LO2, r_kb=3), "dres_kb_rows needs a three-byte dres", name)    # fewer rows than M
    refused(bwd3(D=48, ld=48, r_hi=HI2, r_lo=LO2, r_kb=4), "dres_kb_rows needs a three-byte dres", name)
    refused(bwd3(dxT=None, dx_lo=OLO), "dx_lo needs dxT", name)
    refused(bwd3(dxT=O2 + 4, dx_lo=OLO), "dx_lo needs dxT", name)
    refused(bwd3(dx_lo=OLO + 2), "dx_lo needs dxT", name)
    refused(bwd3(dt=7), "bad dtype", name)

    def per(dt=BF, M=4, D=64, dy=DY, x=X, x_hi=None, x_lo=None, x_kb=0, g=G, eps=1e-5, rows=O1, period=2, dx32=None, dxT=O2, dx_lo=OLO):
        return lib.uia_layernorm_bwd_periodic(None, dt, M, D, dy, x, x_hi, x_lo, x_kb, g, eps, rows, period, dx32, dxT, dx_lo)

    name = "uia_layernorm_bwd_periodic"
    refused(per(period=0), "unsupported shape", name)
    for D in (0, 6, 1028):
        refused(per(D=D), "unsupported shape", name)
    refused(per(rows=None), "null tensor", name)
    refused(per(rows=O1 + 8), "16-byte aligned", name)
    refused(per(dt=7), "bad dtype", name)
    refused(per(dx_lo=None), "writes a three-byte result", name)                              # bf16 without dx_lo
    refused(per(dxT=O2 + 4), "writes a three-byte result", name)
    refused(per(dt=FP, dx32=O2), "three-byte tensors need bf16", name)                         # fp32 with dx_lo
    refused(per(dt=FP, dx32=O2, dx_lo=None, x_hi=HI), "three-byte tensors need bf16", name)    # fp32 with x_hi
    refused(per(x_hi=HI, x_lo=LO), "x as a three-byte tensor", name)
    refused(per(x=None, x_hi=HI, x_lo=LO, x_kb=3), "x as a three-byte tensor", name)
    refused(per(x_kb=4), "x_kb_rows without a three-byte x", name)

    def pool(B=2, L=10, row0=1, n=9, D=64, ldx=64, x=X, g=G, b=B_, eps=1e-6, ws=WS, out=O1, ldo=64):
        return lib.uia_ln_mean_rows(None, B, L, row0, n, D, ldx, x, g, b, eps, ws, out, ldo)

    name = "uia_ln_mean_rows"
    refused(pool(n=10), "outside the 10 tokens", name)                                         # row0 + n > L
    refused(pool(n=0), "outside the", name)
    refused(pool(row0=-1), "outside the", name)
    for D in (0, 6, 1028):
        refused(pool(D=D, ldx=1028, ldo=1028), "must be a multiple of 4", name)
    refused(pool(ldo=60), "leading dimensions", name)
    refused(pool(ldx=60), "leading dimensions", name)
    refused(pool(ldx=66), "leading dimensions", name)
    refused(pool(ws=None), "null tensor", name)
    refused(pool(eps=-1e-6), "eps must be >= 0", name)
    for kw in (dict(x=X + 8), dict(g=G + 4), dict(b=B_ + 8), dict(ws=WS + 8), dict(out=O1 + 8)):
        refused(pool(**kw), "16-byte aligned", name)
