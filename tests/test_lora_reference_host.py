"""CPU only: the host restatement of the LoRA dropout generator (tests/lora_reference.py) against a scalar second form and its own
statistics, every float64 reference against a second independent form, and the bounds of tests/test_lora_contract_gpu.py against
planted bugs at that file's case shapes."""
import itertools
import math

import numpy as np
import pytest
import torch

import lora_reference as R

F64 = R.F64
BF, F32 = torch.bfloat16, torch.float32


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


# ------------------------------------------------------------------------------------------ second form: scalar Python integers
def _hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def _keep8(seed, grp, th):
    h = _hash32((_hash32((grp ^ seed) & 0xFFFFFFFF) + (seed >> 32)) & 0xFFFFFFFF)
    m = 0
    for q in range(4):
        m |= (1 if (h & 0xFFFF) >= th else 0) << (2 * q)
        m |= (1 if (h >> 16) >= th else 0) << (2 * q + 1)
        h ^= (h << 13) & 0xFFFFFFFF
        h ^= h >> 17
        h ^= (h << 5) & 0xFFFFFFFF
    return m


def _keep(seed, idx, th):
    h = _hash32((idx ^ seed) & 0xFFFFFFFF) ^ _hash32(((idx * 0x9E3779B9) & 0xFFFFFFFF) + (seed >> 32))
    return _hash32(h) >= th


def test_derived_seeds_are_those_of_next_seed():
    from uia_hip import functional as UF
    saved = dict(UF._STATE)
    try:
        UF.set_dropout_seed(0x5EED)
        assert [UF._next_seed() for _ in range(4)] == R.derived_seeds(0x5EED, 4)
    finally:
        UF._STATE.update(saved)
    assert len(set(R.SEEDS)) == 9


def test_vectorised_generator_equals_scalar_form():
    G = 4096
    grp = np.concatenate([np.arange(G - 8, dtype=np.uint64), np.array([2 ** 31 - 1, 2 ** 31, 2 ** 32 - 8, 2 ** 32 - 7, 2 ** 32 - 6, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint64)])
    for seed in R.SEEDS:
        for p in (0.1, 0.5, 0.99999):
            th = R.thresh16(p)
            got = R.keep8(seed, grp, th)
            want = np.array([[(_keep8(seed, int(g), th) >> e) & 1 for e in range(8)] for g in grp], dtype=bool)
            assert np.array_equal(got, want), (hex(seed), p)
            mt = R.mona_thresh(p)
            assert np.array_equal(R.keep_elem(seed, grp, mt), np.array([_keep(seed, int(g), mt) for g in grp])), (hex(seed), p)
    assert np.array_equal(R.hash32(grp), np.array([_hash32(int(g)) for g in grp], dtype=np.uint64))


def test_thresholds_and_scale():
    assert [R.thresh16(p) for p in (0.0, 1e-6, 0.1, 0.25, 0.5, 0.9, 0.99999, 1.0)] == [0, 0, 6554, 16384, 32768, 58982, 65535, 65535]
    assert R.thresh16(7.6e-6) == 0 and R.thresh16(7.7e-6) == 1                  # the rounding point 0.5 / 65536
    assert R.mona_thresh(0.0) == 0 and R.mona_thresh(0.5) == 2 ** 31 and R.mona_thresh(0.1) == int(np.float32(0.1) * np.float32(2.0 ** 32))
    assert R.mona_thresh(1.0) == 2 ** 32 - 1
    assert float(R.inv_keep32(0.5)) == 2.0 and float(R.inv_keep32(0.1)) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))
    # p = 1e-6: nothing is dropped, everything is scaled
    assert bool(R.keep_mask(5, 4, 64, 1e-6).all()) and float(R.inv_keep32(1e-6)) > 1.0
    # keep_mask: the window of a wider tensor is the slice of that tensor's mask
    full = R.keep_mask(77, 9, 128, 0.5)
    assert torch.equal(R.keep_mask(77, 9, 64, 0.5, ld=128, col0=8), full[:, 8:72])
    assert torch.equal(R.keep_mask(77, 1, 9 * 128, 0.5).reshape(9, 128), full)


def test_fma32_is_correctly_rounded():
    from fractions import Fraction
    g = np.random.default_rng(3)
    a = g.standard_normal(4000).astype(np.float32)
    b = np.full(4000, R.inv_keep32(0.1), dtype=np.float32)
    c = (g.standard_normal(4000) * np.exp2(g.integers(-30, 4, 4000))).astype(np.float32)
    # ties of the float64 sum: c a multiple of 2^-24 beside a product with bits far below
    a[:8], b[:8], c[:8] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24) * np.arange(1, 9, dtype=np.float32)
    got = R.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r = float(got[i])
        lo, hi = float(np.nextafter(got[i], np.float32(-np.inf))), float(np.nextafter(got[i], np.float32(np.inf)))
        assert abs(exact - Fraction(r)) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi))), i


# ------------------------------------------------------------------------------------------ statistics
def _z_rate(k, n, q):
    return (k - n * q) / math.sqrt(n * q * (1 - q))


def _z_corr(a, b):
    """z-score of the sample correlation of two boolean arrays (r·√n is standard normal for independent draws)."""
    a, b = a.reshape(-1), b.reshape(-1)
    n = a.size
    sa, sb, sab = float(a.sum()), float(b.sum()), float((a & b).sum())
    cov = sab / n - (sa / n) * (sb / n)
    return cov / math.sqrt((sa / n) * (1 - sa / n) * (sb / n) * (1 - sb / n)) * math.sqrt(n)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_generator_statistics(p):
    G = 1 << 20
    seeds = R.derived_seeds(0x5EED, 4)
    q = R.keep_rate(p)
    th = R.thresh16(p)
    grp = np.arange(G, dtype=np.uint64)
    masks = [R.keep8(s, grp, th) for s in seeds]
    z = {}
    for si, m in enumerate(masks):
        z[f"seed {si} overall rate"] = _z_rate(float(m.sum()), m.size, q)
        for e in range(8):
            z[f"seed {si} bit {e} rate"] = _z_rate(float(m[:, e].sum()), G, q)
        pairs = {(i, j): _z_corr(m[:, i], m[:, j]) for i, j in itertools.combinations(range(8), 2)}
        worst = max(pairs, key=lambda k: abs(pairs[k]))
        z[f"seed {si} bits {worst} (largest pairwise)"] = pairs[worst]
        z[f"seed {si} adjacent groups"] = _z_corr(m[:-1], m[1:])
        z[f"seed {si} bit 7 and the next group's bit 0"] = _z_corr(m[:-1, 7], m[1:, 0])
        z[f"seed {si} one row apart at width 768"] = _z_corr(m[:-96], m[96:])
    for i, j in itertools.combinations(range(4), 2):
        z[f"seeds {i}, {j}"] = _z_corr(masks[i], masks[j])
    worst = max(z, key=lambda k: abs(z[k]))
    print(f"p={p}: worst |z| {abs(z[worst]):.2f} at {worst}")
    bad = {k: round(v, 2) for k, v in z.items() if not abs(v) <= 5}
    assert not bad, bad


# ------------------------------------------------------------------------------------------ cross-checks against a second form
def test_references_equal_second_forms():
    M, K, N, D = 37, 64, 128, 768
    p, seed = 0.25, R.SEEDS[5]
    inv = float(R.inv_keep32(p))
    # dropout: keep·x·inv, the unfused form (accumulate = 0: the fma adds zero)
    x = rnd(8 * 257, seed=1).to(BF)
    vals, keep = R.dropout(x, p, seed)
    assert torch.equal(vals, torch.where(keep, (x.float() * torch.tensor(inv, dtype=F32)), torch.zeros(())).to(BF))
    assert torch.equal(keep.reshape(-1), torch.from_numpy(R.keep8(seed, np.arange(257), R.thresh16(p)).reshape(-1)))
    x32, d0 = rnd(8 * 257, seed=2), rnd(8 * 257, seed=3)
    acc, _ = R.dropout(x32, p, seed, True, d0)
    two = d0.double() + x32.double() * torch.where(keep, torch.tensor(inv, dtype=F64), torch.zeros((), dtype=F64))
    assert float((acc.double() - two).abs().max()) <= 2.0 ** -24 * float(two.abs().max())
    assert torch.equal(acc[~keep], d0[~keep])
    # gemm_drop_a: einsum over the masked, scaled operand
    a, w, bias = rnd(M, 320, seed=4).to(BF), rnd(64, 320, seed=5).to(BF), rnd(64, seed=6)
    (t, ad), mag = R.gemm_drop_a(a, w, bias, p, seed)
    km = R.keep_mask(seed, M, 320, p)
    assert torch.equal(ad, R.dropped(a, p, km))
    want = torch.einsum("mk,nk->mn", ad.double(), w.double()) + bias.double()
    assert bool(((t - want).abs() <= 1e-12 * mag).all())
    # gemm_drop_acc: F.linear and torch's own masking
    a, w = rnd(M, K, seed=7).to(BF), rnd(N, K, seed=8).to(BF)
    resid = rnd(M, N, seed=9).to(BF)
    ref, mag, keep = R.gemm_drop_acc(a, w, 1.75, bias=None, p=p, seed=seed, resid=resid)
    want = resid.double() + torch.nn.functional.linear(a.double(), w.double()) * 1.75 * inv * keep.double()
    assert bool(((ref - want).abs() <= 1e-12 * mag).all())
    assert torch.equal(ref[~keep], resid.double()[~keep])
    # wgrad: per-row outer products summed, on the valid extent
    a, b, dw0, db0 = rnd(130, 64, seed=10).to(BF), rnd(130, 64, seed=11).to(BF), rnd(5, 7, seed=12), rnd(5, seed=13)
    kb = R.keep_mask(seed, 130, 64, p, ld=128, col0=8)
    r = R.wgrad(a, b, 0.5, dw0, 5, 7, drop=(p, kb), dbias0=db0)
    bd = torch.where(kb, b.float() * torch.tensor(inv, dtype=F32), torch.zeros(())).to(BF).double()
    want = dw0.double() + 0.5 * torch.einsum("mi,mj->ij", a.double()[:, :5], bd[:, :7])
    assert bool(((r["dw"] - want).abs() <= 1e-12 * r["mag_dw"]).all())
    assert bool(((r["db"] - (db0.double() + a.double()[:, :5].sum(0))).abs() <= 1e-12 * r["mag_db"]).all())
    # lora_rank_update: one concatenated product over the sources
    qs = [rnd(M, 64, seed=20 + i).to(BF) for i in range(3)]
    ws = [rnd(256, 64, seed=30 + i).to(BF) for i in range(3)]
    out0 = rnd(M, 256, seed=40).to(BF)
    ref, mag = R.lora_rank_update(out0, qs, ws, 1.5, 0.0, None)
    want = out0.double() + 1.5 * torch.cat(qs, 1).double() @ torch.cat(ws, 1).double().T
    assert bool(((ref - want).abs() <= 1e-12 * mag).all())
    keeps = [R.keep_mask(R.SEEDS[5 + i], M, 256, p) for i in range(3)]
    ref, mag = R.lora_rank_update(out0, qs, ws, 1.5, p, keeps)
    want = out0.double() + sum(1.5 * inv * (q.double() @ w_.double().T) * k.double() for q, w_, k in zip(qs, ws, keeps))
    assert bool(((ref - want).abs() <= 1e-12 * mag).all())
    # ln_lora_down: F.layer_norm; the product against torch's matmul of the masked operand
    x, gamma, beta = rnd(M, D, seed=50, shift=100.0), rnd(D, seed=51, scale=0.5, shift=1.0), rnd(D, seed=52)
    a_rows = [rnd(16, D, seed=60 + i).to(BF) for i in range(2)]
    hk = R.layernorm_torch(x, gamma, beta, 1e-5).to(BF)
    keeps = [R.keep_mask(R.SEEDS[5 + i], M, D, p) for i in range(2)]
    (h, mag_h), ts = R.ln_lora_down(x, gamma, beta, 1e-5, hk, a_rows, p, keeps)
    assert bool(((h - R.layernorm_torch(x, gamma, beta, 1e-5)).abs() <= 1e-12 * mag_h).all())
    for (t, mag), a_, k in zip(ts, a_rows, keeps):
        want = (hk.float() * torch.tensor(inv, dtype=F32) * k).to(BF).double() @ a_.double().T
        assert bool(((t - want).abs() <= 1e-12 * mag).all())


# ------------------------------------------------------------------------------------------ planted bugs
def _ratio(got, ref, mag, c, dt):
    ck = R.Checker()
    return ck.check("planted", got, ref, R.bound(ref, mag, c, dt), "")


def _planted_cases():
    """(name, error/bound of the planted kernel) at the case shapes of test_lora_contract_gpu.py.  A planted kernel is the float64
    value of the buggy computation rounded to the output's dtype."""
    out = []
    p = 0.5
    seeds = R.derived_seeds(0x5EED, 4)
    inv = float(R.inv_keep32(p))
    # -- wgrad with the window: mask indexed with the leading dimension ldb instead of drop_ld (here: the logical width J of the window
    #    taken for the row stride of the dropped tensor)
    for M in R.WGRAD_M[1:]:
        for I, J in R.WGRAD_IJ:
            a, b, dw0 = rnd(M, I, seed=M + I).to(BF), rnd(M, J, seed=M + J + 1).to(BF), rnd(I, J, seed=3)
            keep = R.keep_mask(seeds[0], M, J, p, ld=J + 64, col0=8)
            r = R.wgrad(a, b, 1.0, dw0, drop=(p, keep))
            bug = R.wgrad(a, b, 1.0, dw0, drop=(p, R.keep_mask(seeds[0], M, J, p, ld=J, col0=0)))
            out.append((f"wgrad M={M} {I}x{J}: mask indexed with the wrong row stride", _ratio(bug["dw"].float(), r["dw"], r["mag_dw"], R.C_WGRAD, F32)))
            # a tail row counted twice (the clamped duplicate of row M - 1 not zeroed)
            twice = r["dw"] + a.double()[M - 1:M].T @ R.dropped(b, p, keep).double()[M - 1:M]
            out.append((f"wgrad M={M} {I}x{J}: tail row counted twice", _ratio(twice.float(), r["dw"], r["mag_dw"], R.C_WGRAD, F32)))
            # problem s of a group using the seed of problem s + 1
            nxt = R.wgrad(a, b, 1.0, dw0, drop=(p, R.keep_mask(seeds[1], M, J, p, ld=J + 64, col0=8)))
            out.append((f"wgrad M={M} {I}x{J}: the neighbour's seed", _ratio(nxt["dw"].float(), r["dw"], r["mag_dw"], R.C_WGRAD, F32)))
            # a missing 1 / (1 - p)
            b_unscaled = torch.where(keep, b, torch.zeros((), dtype=BF))
            miss = dw0.double() + a.double().T @ b_unscaled.double()
            out.append((f"wgrad M={M} {I}x{J}: missing 1/(1-p)", _ratio(miss.float(), r["dw"], r["mag_dw"], R.C_WGRAD, F32)))
    # -- N = 64 stream GEMM: the second eight columns of a 16-column piece reuse the first draw; a missing scale
    for M in R.GEMM_A_M:
        for K in R.GEMM_A_K:
            a, w = rnd(M, K, seed=M + K).to(BF), rnd(64, K, seed=K).to(BF)
            (t, ad), mag = R.gemm_drop_a(a, w, None, p, seeds[0])
            keep = R.keep_mask(seeds[0], M, K, p)
            k2 = keep.reshape(M, K // 16, 2, 8).clone()
            k2[:, :, 1] = k2[:, :, 0]
            bug = R.dropped(a, p, k2.reshape(M, K)).double() @ w.double().T
            out.append((f"gemm_drop_a M={M} K={K}: second eight columns reuse the first draw", _ratio(bug.to(BF), t, mag, R.C_GEMM_DROP_A, BF)))
            miss = torch.where(keep, a, torch.zeros((), dtype=BF)).double() @ w.double().T
            out.append((f"gemm_drop_a M={M} K={K}: missing 1/(1-p)", _ratio(miss.to(BF), t, mag, R.C_GEMM_DROP_A, BF)))
    # -- K = 64 stream GEMM: the same two on the accumulator
    for M in R.GEMM_ACC_M:
        for N in R.GEMM_ACC_N:
            a, w, resid = rnd(M, 64, seed=M + N).to(BF), rnd(N, 64, seed=N).to(BF), rnd(M, N, seed=5).to(BF)
            ref, mag, keep = R.gemm_drop_acc(a, w, 1.75, None, p, seeds[0], resid)
            k2 = keep.reshape(M, N // 16, 2, 8).clone()
            k2[:, :, 1] = k2[:, :, 0]
            v = 1.75 * inv * (a.double() @ w.double().T)
            bug = resid.double() + torch.where(k2.reshape(M, N), v, torch.zeros_like(v))
            out.append((f"gemm_drop_acc M={M} N={N}: second eight columns reuse the first draw", _ratio(bug.to(BF), ref, mag, R.C_GEMM_DROP_ACC, BF)))
            miss = resid.double() + torch.where(keep, v / inv, torch.zeros_like(v))
            out.append((f"gemm_drop_acc M={M} N={N}: missing 1/(1-p)", _ratio(miss.to(BF), ref, mag, R.C_GEMM_DROP_ACC, BF)))
    # -- lora_rank_update: source s with the seed of source s + 1; mask indexed with ldo instead of N
    for M in R.RANK_M:
        for N in R.RANK_N:
            qs = [rnd(M, 64, seed=M + i).to(BF) for i in range(2)]
            ws = [rnd(N, 64, seed=N + i).to(BF) for i in range(2)]
            out0 = rnd(M, N, seed=7).to(BF)
            keeps = [R.keep_mask(seeds[i], M, N, 0.25) for i in range(2)]
            ref, mag = R.lora_rank_update(out0, qs, ws, 1.5, 0.25, keeps)
            bug, _ = R.lora_rank_update(out0, qs, ws, 1.5, 0.25, [R.keep_mask(seeds[i + 1], M, N, 0.25) for i in range(2)])
            out.append((f"lora_rank_update M={M} N={N}: the neighbour's seed", _ratio(bug.to(BF), ref, mag, R.C_RANK, BF)))
            if M > 1:
                bug, _ = R.lora_rank_update(out0, qs, ws, 1.5, 0.25, [R.keep_mask(seeds[i], M, N, 0.25, ld=N + 64) for i in range(2)])
                out.append((f"lora_rank_update M={M} N={N}: mask indexed with the leading dimension", _ratio(bug.to(BF), ref, mag, R.C_RANK, BF)))
    # -- ln_lora_down: the neighbour's seed; columns r..15 of t non-zero for rank r < 16 (the exact-zero comparison: any non-zero value fails)
    for D in R.LN_D:
        for M in R.LN_M:
            x, gamma, beta = rnd(M, D, seed=M + D), rnd(D, seed=D, scale=0.5, shift=1.0), rnd(D, seed=D + 1)
            hk = R.layernorm_torch(x, gamma, beta, 1e-5).to(BF)
            a_rows = [rnd(16, D, seed=70 + i).to(BF) for i in range(2)]
            keeps = [R.keep_mask(seeds[i], M, D, 0.1) for i in range(2)]
            _, ts = R.ln_lora_down(x, gamma, beta, 1e-5, hk, a_rows, 0.1, keeps)
            _, tb = R.ln_lora_down(x, gamma, beta, 1e-5, hk, a_rows, 0.1, [R.keep_mask(seeds[i + 1], M, D, 0.1) for i in range(2)])
            out.append((f"ln_lora_down M={M} D={D}: the neighbour's seed", _ratio(tb[0][0].to(BF), ts[0][0], ts[0][1], R.C_LN_T, BF)))
            if M > 1:
                _, tb = R.ln_lora_down(x, gamma, beta, 1e-5, hk, a_rows, 0.1, [R.keep_mask(seeds[i], M, D, 0.1, ld=D + 8) for i in range(2)])
                out.append((f"ln_lora_down M={M} D={D}: mask indexed with the leading dimension", _ratio(tb[0][0].to(BF), ts[0][0], ts[0][1], R.C_LN_T, BF)))
    return out


def test_planted_bugs_exceed_the_bounds():
    missed = [(name, round(r, 3)) for name, r in _planted_cases() if not r > 1.0]
    assert not missed, missed


def test_nonzero_rank_padding_fails_the_exact_comparison():
    """Columns r..15 of t for rank r < 16 are compared exactly with zero: the smallest bf16 there is a failure."""
    ck = R.Checker()
    t = torch.zeros(5, 64, dtype=BF)
    ck.exact("t padding", t[:, 8:], torch.zeros(5, 56, dtype=BF), "clean")
    assert ck.ok()
    t[3, 9] = 2.0 ** -126
    ck.exact("t padding", t[:, 8:], torch.zeros(5, 56, dtype=BF), "planted")
    assert not ck.ok()
