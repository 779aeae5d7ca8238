"""-m gpu: what ops.attn_fwd / ops.attn_bwd (uia_attn_fwd, uia_attn_bwd[_cfg]) must compute, at every length, mask, dtype, head dim
and kernel path, judged element-wise against the float64 reference of tests/attn_reference.py on the operands the kernel sees.

Each test loops over its cases and collects every failing comparison (bar, case, worst (b, h, row), error/bound) before it fails
once with the list.  The bars and their calibrated constants are in attn_reference.py."""
import math

import pytest
import torch

import attn_reference as R

pytestmark = pytest.mark.gpu

B, H = 3, 2
MASKS = ("none", "causal", "keypad")
# lengths next to every forward instantiation (<5,4> to 80, <13,7> to 208, <16,8> to 256, <17,8> to 272), the backward's LDS / tile
# switches (240, 256) and its longest accepted length
EDGES = (1, 2, 16, 17, 80, 81, 128, 129, 208, 209, 240, 241, 256, 257, 272, 288)
DT = (torch.bfloat16, torch.float32)


@pytest.fixture(scope="module")
def ops():
    from uia_hip import ops as o
    return o


@pytest.fixture(scope="module")
def UiaError():
    from uia_hip._lib import UiaError as E
    return E


def dev():
    return torch.device("cuda:0")


def keylens(L):
    """keylen per batch row, drawn from {1, 15, 16, 17, L-1, L, L+5} (L-1 = 0 at L = 1 and L+5 exercise the clamp to [1, L])."""
    ch = (1, 15, 16, 17, L - 1, L, L + 5)
    return torch.tensor([ch[(L + 3 * b) % 7] for b in range(B)], dtype=torch.int32, device=dev())


def fused(L, dt, dh=64, seed=0, nb=B):
    g = torch.Generator(device=dev()).manual_seed(seed * 1000 + L)
    return (torch.randn(nb * L, 3 * H * dh, device=dev(), generator=g) * 1.5).to(dt)


def split(qkv, dh=64):
    D = H * dh
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]


def nan_like(rows, cols, dt):
    return torch.full((rows, cols), float("nan"), device=dev(), dtype=dt)


def run_fwd(ops, qkv, L, dt, mask, keylen, dh=64, scale=None):
    q, k, v = split(qkv, dh)
    out = nan_like(B * L, H * dh, dt)
    lse = torch.full((B, H, L), float("nan"), device=dev())
    ops.attn_fwd(q, k, v, out, B, H, L, lse=lse, mask=mask, keylen=keylen, scale=scale)
    return out, lse


def run_bwd(ops, qkv, out, dout, lse, L, dt, mask, keylen, dh=64, cfg=None, scale=None):
    q, k, v = split(qkv, dh)
    D = H * dh
    d = nan_like(B * L, 3 * D, dt)                 # NaN-filled: an element the kernel does not write fails its bound
    ops.attn_bwd(q, k, v, out, dout, lse, d[:, :D], d[:, D:2 * D], d[:, 2 * D:], B, H, L, mask=mask, keylen=keylen, scale=scale, dh=dh, cfg=cfg)
    return d[:, :D], d[:, D:2 * D], d[:, 2 * D:]


def ref_of(qkv, L, mask, keylen, dh=64, scale=None, dout=None):
    q, k, v = (R.heads(t, B, L, H, dh) for t in split(qkv, dh))
    if dout is None:
        return R.fwd(q, k, v, mask, keylen, scale)
    return R.bwd(q, k, v, R.heads(dout, B, L, H, dh), mask, keylen, scale)


def check_fwd(chk, out, lse, ref, L, dt, ctx, dh=64, tag=""):
    o = R.heads(out, B, L, H, dh)
    chk.check(f"out{tag} {dt}", o, ref["out"], R.out_bound(ref["out"], ref["pabsv"], dt), ctx)
    if lse is not None:
        chk.check(f"lse{tag} {dt}", lse, ref["lse"], R.lse_bound(ref["lse"], dt), ctx)


def check_bwd(chk, grads, ref, L, dt, ctx, dh=64, tag=""):
    for name, g in zip(("dq", "dk", "dv"), grads):
        chk.check(f"{name}{tag} {dt}", R.heads(g, B, L, H, dh), ref[name], R.grad_bound(ref[name], ref["mag_" + name], dt), ctx)


def finish(chk):
    print("\n" + chk.report(0))
    assert chk.ok(), chk.report()


def dout_for(L, dt, dh=64):
    g = torch.Generator(device=dev()).manual_seed(7 + L)
    return torch.randn(B * L, H * dh, device=dev(), generator=g).to(dt)


def bwd_inputs(ops, qkv, L, dt, mask, keylen, dh=64):
    """out and lse for the backward: the kernel's own forward where it exists, else (bf16 273 <= L <= 288) the reference's, rounded as stored."""
    if L <= 272 or dh != 64:
        return run_fwd(ops, qkv, L, dt, mask, keylen, dh)
    f = ref_of(qkv, L, mask, keylen, dh)
    return R.rows(f["out"]).to(dt), f["lse"].float()


# ---------------------------------------------------------------- a. forward length sweep

@pytest.mark.parametrize("dt", DT)
def test_forward_length_sweep(ops, dt):
    chk = R.Checker()
    for L in range(1, 273):
        qkv = fused(L, dt)
        for mask in MASKS:
            kl = keylens(L) if mask == "keypad" else None
            out, lse = run_fwd(ops, qkv, L, dt, mask, kl)
            check_fwd(chk, out, lse, ref_of(qkv, L, mask, kl), L, dt, f"fwd L={L} mask={mask} keylen={None if kl is None else kl.tolist()}")
    finish(chk)


# ---------------------------------------------------------------- b. backward length sweep

@pytest.mark.parametrize("dt", DT)
def test_backward_length_sweep(ops, dt):
    """Default configuration, every accepted length.  NaN-filled gradients: every element written; masked keys: dk = dv = 0 exactly
    (their reference and magnitude are 0, so the bound is 0)."""
    chk = R.Checker()
    for L in range(1, (288 if dt == torch.bfloat16 else 272) + 1):
        qkv, dout = fused(L, dt, seed=1), dout_for(L, dt)
        for mask in MASKS:
            kl = keylens(L) if mask == "keypad" else None
            out, lse = bwd_inputs(ops, qkv, L, dt, mask, kl)
            grads = run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl)
            check_bwd(chk, grads, ref_of(qkv, L, mask, kl, dout=dout), L, dt, f"bwd L={L} mask={mask} keylen={None if kl is None else kl.tolist()}")
    finish(chk)


def test_backward_configs(ops, UiaError):
    """uia_attn_bwd_cfg 1-7 at the lengths next to each instantiation and LDS switch.  The persistent kernel (cfg 5) holds 15 tiles
    (240 tokens) and must refuse longer heads; every other configuration takes the bf16 backward's whole range."""
    dt, chk, missing = torch.bfloat16, R.Checker(), []
    for L in EDGES:
        qkv, dout = fused(L, dt, seed=2), dout_for(L, dt)
        for mask in MASKS:
            kl = keylens(L) if mask == "keypad" else None
            out, lse = bwd_inputs(ops, qkv, L, dt, mask, kl)
            ref = ref_of(qkv, L, mask, kl, dout=dout)
            for cfg in range(1, 8):
                if cfg == 5 and L > 240:
                    try:
                        run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl, cfg=cfg)
                        missing.append(f"cfg {cfg} L={L} mask={mask}: accepted, expected UiaError")
                    except UiaError:
                        pass
                    continue
                grads = run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl, cfg=cfg)
                check_bwd(chk, grads, ref, L, dt, f"bwd cfg={cfg} L={L} mask={mask}")
    assert not missing, missing
    finish(chk)


# ---------------------------------------------------------------- c. structured inputs with exact answers

def structured(L, dt, dh=64, seed=3):
    """fused qkv with K = 0 and V[j, (j + h) mod dh] = w_j (exact in bf16), Q random."""
    qkv = fused(L, dt, dh, seed)
    D = H * dh
    qkv[:, D:2 * D] = 0
    qkv[:, 2 * D:] = R.rows(R.structured_v(B, H, L, dh, dev())).to(dt)
    return qkv


@pytest.mark.parametrize("dt", DT)
def test_structured_exact(ops, dt):
    """Forward at every length: out is the mean of the visible V rows to one rounding, lse = log n.  Backward: dq = 0 exactly,
    dv_j = Σ_{i sees j} dO_i / n_i and dk from its closed form, within the gradient bars."""
    chk = R.Checker()
    for L in range(1, (288 if dt == torch.bfloat16 else 272) + 1):
        qkv = structured(L, dt)
        dout = dout_for(L, dt)
        for mask in MASKS:
            kl = keylens(L) if mask == "keypad" else None
            q, _, v = (R.heads(t, B, L, H, 64) for t in split(qkv))
            o_ref, lse_ref = R.closed_fwd(v, mask, kl)
            ctx = f"structured L={L} mask={mask} keylen={None if kl is None else kl.tolist()}"
            if L <= 272:
                out, lse = run_fwd(ops, qkv, L, dt, mask, kl)
                chk.check(f"out exact {dt}", R.heads(out, B, L, H, 64), o_ref, R.one_rounding_bound(o_ref, dt), ctx)
                chk.check(f"lse exact {dt}", lse, lse_ref, R.lse_exact_bound(lse_ref), ctx)
            else:
                out, lse = R.rows(o_ref).to(dt), lse_ref.float()
            dq, dk, dv = run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl)
            dq_ref, dk_ref, dv_ref = R.closed_bwd(q, v, R.heads(dout, B, L, H, 64), mask, kl)
            ref = ref_of(qkv, L, mask, kl, dout=dout)          # magnitudes for the bounds
            chk.check(f"dq exact {dt}", R.heads(dq, B, L, H, 64), dq_ref, torch.zeros_like(dq_ref), ctx)
            chk.check(f"dk closed {dt}", R.heads(dk, B, L, H, 64), dk_ref, R.grad_bound(dk_ref, ref["mag_dk"], dt), ctx)
            chk.check(f"dv closed {dt}", R.heads(dv, B, L, H, 64), dv_ref, R.grad_bound(dv_ref, ref["mag_dv"], dt), ctx)
    finish(chk)


# ---------------------------------------------------------------- d. invariances

def bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


@pytest.mark.parametrize("dt", DT)
def test_masked_keys_do_not_matter(ops, dt):
    """Keys a query cannot see are never read into its result: rewriting the K and V rows of padded keys (keypad) or of keys past a
    pivot (causal) with large finite values leaves out, lse, dq and the visible rows of dk / dv bit-identical.  A kernel that took
    the row max over masked scores would underflow every visible exponential here."""
    bad = []
    big = 3.0e4
    for L in EDGES[:-1]:
        D = H * 64
        qkv, dout = fused(L, dt, seed=4), dout_for(L, dt)
        kl = keylens(L)
        out0, lse0 = run_fwd(ops, qkv, L, dt, "keypad", kl)
        g0 = run_bwd(ops, qkv, out0, dout, lse0, L, dt, "keypad", kl)
        alt = qkv.clone().view(B, L, 3 * D)
        for b, n in enumerate(R.clamp_keylen(kl, L).tolist()):
            alt[b, n:, D:] = big * torch.sign(alt[b, n:, D:] + 0.5)
        alt = alt.view(B * L, 3 * D)
        out1, lse1 = run_fwd(ops, alt, L, dt, "keypad", kl)
        g1 = run_bwd(ops, alt, out1, dout, lse1, L, dt, "keypad", kl)
        seen = (torch.arange(L, device=dev())[None, :] < R.clamp_keylen(kl, L)[:, None].to(dev())).reshape(B * L)
        same = [("out", out0, out1), ("lse", lse0, lse1), ("dq", g0[0], g1[0]), ("dk visible", g0[1][seen], g1[1][seen]), ("dv visible", g0[2][seen], g1[2][seen])]
        bad += [f"keypad L={L}: {n} changed" for n, a, c in same if not torch.equal(bits(a), bits(c))]
        out0, lse0 = run_fwd(ops, qkv, L, dt, "causal", None)
        for t in sorted({0, 15, 16, L // 2, L - 2}):
            if not 0 <= t < L - 1:
                continue
            alt = qkv.clone().view(B, L, 3 * D)
            alt[:, t + 1:, D:] = big * torch.sign(alt[:, t + 1:, D:] + 0.5)
            out1, lse1 = run_fwd(ops, alt.view(B * L, 3 * D), L, dt, "causal", None)
            rows_ = (torch.arange(L, device=dev()) <= t).repeat(B)
            if not torch.equal(bits(out0[rows_]), bits(out1[rows_])) or not torch.equal(bits(lse0[..., :t + 1]), bits(lse1[..., :t + 1])):
                bad.append(f"causal L={L}: rows <= {t} changed when keys > {t} did")
    assert not bad, bad


@pytest.mark.parametrize("dt", DT)
def test_score_offset_and_scale(ops, dt):
    """A common vector added to every key of a head moves each row's scores by up to ~80: out must still match the reference of the
    shifted operands, finite.  A non-default scale (forward and backward) must match the reference with that scale."""
    chk = R.Checker()
    D = H * 64
    for L in EDGES[:-1]:
        qkv = fused(L, dt, seed=5)
        q = R.heads(qkv[:, :D], B, L, H, 64)
        for h in range(H):
            qs = q[:, h].sum(-1).abs().max() / 8.0                    # largest row of q·1·scale
            qkv[:, D + h * 64:D + (h + 1) * 64] = (qkv[:, D + h * 64:D + (h + 1) * 64].float() + float(80.0 / qs)).to(dt)
        for mask in MASKS:
            kl = keylens(L) if mask == "keypad" else None
            out, _ = run_fwd(ops, qkv, L, dt, mask, kl)
            f = ref_of(qkv, L, mask, kl)
            chk.check(f"out offset {dt}", R.heads(out, B, L, H, 64), f["out"], R.out_bound(f["out"], f["pabsv"], dt, R.C_OUT_OFFSET[dt]), f"offset L={L} mask={mask}")
        qkv, dout = fused(L, dt, seed=6), dout_for(L, dt)
        for scale in (0.03, 0.37):
            for mask in MASKS:
                kl = keylens(L) if mask == "keypad" else None
                out, lse = run_fwd(ops, qkv, L, dt, mask, kl, scale=scale)
                ref = ref_of(qkv, L, mask, kl, scale=scale, dout=dout)
                check_fwd(chk, out, lse, ref, L, dt, f"scale={scale} L={L} mask={mask}")
                check_bwd(chk, run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl, scale=scale), ref, L, dt, f"scale={scale} L={L} mask={mask}")
    finish(chk)


# ---------------------------------------------------------------- e. writes stay inside the output

G = 3             # guard rows before and after every output


def sentinel(shape, dt):
    t = torch.empty(shape, device=dev(), dtype=dt)
    bits(t).fill_(0x7FC5 if dt == torch.bfloat16 else 0x7FC00005)    # a NaN with a payload no kernel writes
    return t


def guarded(rows, cols, pad, dt, parts=1):
    """A sentinel-filled buffer with G guard rows on each side and `pad` guard columns after each of `parts` column blocks;
    returns (buffer, the part views [rows, cols] with row pitch parts*(cols+pad))."""
    buf = sentinel((rows + 2 * G, parts * (cols + pad)), dt)
    return buf, [buf[G:G + rows, i * (cols + pad):i * (cols + pad) + cols] for i in range(parts)]


def untouched(buf, views, dt):
    """True when every element of buf outside the views still holds the sentinel."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=dev())
    for v in views:
        r0 = (v.storage_offset() - buf.storage_offset()) // buf.stride(0)
        c0 = (v.storage_offset() - buf.storage_offset()) % buf.stride(0)
        mask[r0:r0 + v.shape[0], c0:c0 + v.shape[1]] = False
    return torch.equal(bits(buf[mask]), bits(sentinel(buf[mask].shape, dt)))


@pytest.mark.parametrize("dt", DT)
def test_writes_stay_inside(ops, dt):
    """out / lse / dq / dk / dv written into sentinel buffers with guard rows and a row pitch wider than H·dh: every valid element
    written (and right), every guard element untouched.  Dense forward and backward (dh 64), packed forward, small-head path (dh 16, 32)."""
    chk, bad = R.Checker(), []
    pad = 8 if dt == torch.bfloat16 else 4                            # 16 bytes: keeps the rows aligned as the kernels require
    for dh, lengths in ((64, (1, 17, 80, 81, 208, 209, 256, 257, 272)), (16, (17, 197, 513)), (32, (17, 197))):
        D = H * dh
        for L in lengths:
            qkv, dout = fused(L, dt, dh, seed=8), dout_for(L, dt, dh)
            q, k, v = split(qkv, dh)
            for mask in MASKS:
                kl = keylens(L) if mask == "keypad" else None
                ctx = f"guarded dh={dh} L={L} mask={mask}"
                obuf, (out,) = guarded(B * L, D, pad, dt)
                lbuf = sentinel((B * H * L + 2 * G,), torch.float32)
                lse = lbuf[G:G + B * H * L].view(B, H, L)
                ops.attn_fwd(q, k, v, out, B, H, L, lse=lse, mask=mask, keylen=kl, dh=dh)
                ref = ref_of(qkv, L, mask, kl, dh, dout=dout)
                check_fwd(chk, out, lse, ref, L, dt, ctx, dh, tag=f" dh{dh}")
                if not untouched(obuf, [out], dt):
                    bad.append(f"{ctx}: forward wrote outside out")
                if not torch.equal(bits(lbuf[:G]), bits(sentinel((G,), torch.float32))) or not torch.equal(bits(lbuf[-G:]), bits(sentinel((G,), torch.float32))):
                    bad.append(f"{ctx}: forward wrote outside lse")
                gbuf, (dq, dk, dv) = guarded(B * L, D, pad, dt, parts=3)
                ops.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, L, mask=mask, keylen=kl, dh=dh)
                check_bwd(chk, (dq, dk, dv), ref, L, dt, ctx, dh, tag=f" dh{dh}")
                if not untouched(gbuf, [dq, dk, dv], dt):
                    bad.append(f"{ctx}: backward wrote outside dq / dk / dv")
    for lens in ((1, 15, 16, 17, 77, 200, 256), (272, 3, 100, 33)):
        cu, T = packed_cu(lens)
        qkv = packed_tokens(T, dt)
        q, k, v = split(qkv)
        obuf, (out,) = guarded(T, H * 64, pad, dt)
        ops.attn_fwd(q, k, v, out, len(lens), H, max(lens), cu_seqlens=cu)
        if not untouched(obuf, [out], dt):
            bad.append(f"packed {lens}: forward wrote outside out")
    assert not bad, bad
    finish(chk)


# ---------------------------------------------------------------- f. packed cu_seqlens forward

def packed_cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=dev()), cu[-1]


def packed_tokens(T, dt):
    g = torch.Generator(device=dev()).manual_seed(9 + T)
    return (torch.randn(T, 3 * H * 64, device=dev(), generator=g) * 1.5).to(dt)


@pytest.mark.parametrize("dt", DT)
def test_packed_forward(ops, UiaError, dt):
    """Each packed sequence against its own reference (masks none and causal); the unmasked result against the dense key-padding
    launch over the same tokens (rows < keylen); rows outside the packed range untouched; lse or keypad with cu_seqlens refused."""
    chk, bad = R.Checker(), []
    D = H * 64
    for lens in ((1, 15, 16, 17, 77, 200, 256), (272, 3, 100, 33), (208, 209, 80, 81)):
        nb, Lmax = len(lens), max(lens)
        cu, T = packed_cu(lens)
        qkv = packed_tokens(T, dt)
        q, k, v = split(qkv)
        for mask in ("none", "causal"):
            obuf, (out,) = guarded(T, D, 0, dt)
            ops.attn_fwd(q, k, v, out, nb, H, Lmax, mask=mask, cu_seqlens=cu)
            ref, pabsv = R.fwd_packed(q, k, v, cu.tolist(), H, 64, mask)
            view = lambda t: t.view(1, T, H, 64).permute(0, 2, 1, 3)  # noqa: E731  ([1, H, T, dh]: rows are the packed tokens)
            chk.check(f"out packed {dt}", view(out.to(R.F64)), view(ref), view(R.out_bound(ref, pabsv, dt)), f"packed {lens} mask={mask}")
            if not untouched(obuf, [out], dt):
                bad.append(f"packed {lens} mask={mask}: rows outside the packed range written")
        # the dense key-padding launch over the same tokens: sequence b in rows b*Lmax .. b*Lmax+len-1, the rest of the rows random
        dense = fused(Lmax, dt, seed=10, nb=nb)
        for b, n in enumerate(lens):
            dense[b * Lmax:b * Lmax + n] = qkv[int(cu[b]):int(cu[b]) + n]
        kl = torch.tensor(lens, dtype=torch.int32, device=dev())
        dout_ = nan_like(nb * Lmax, D, dt)
        dq, dk, dv = split(dense)
        ops.attn_fwd(dq, dk, dv, dout_, nb, H, Lmax, mask="keypad", keylen=kl)
        out = torch.empty(T, D, device=dev(), dtype=dt)
        ops.attn_fwd(q, k, v, out, nb, H, Lmax, cu_seqlens=cu)
        ref, pabsv = R.fwd_packed(q, k, v, cu.tolist(), H, 64)
        sel = torch.cat([torch.arange(b * Lmax, b * Lmax + n) for b, n in enumerate(lens)]).to(dev())
        view = lambda t: t.view(1, T, H, 64).permute(0, 2, 1, 3)  # noqa: E731
        chk.check(f"packed vs keypad {dt}", view(out.to(R.F64)), view(dout_[sel].to(R.F64)), view(R.out_bound(ref, pabsv, dt)), f"packed vs dense {lens}")
        lse = torch.empty(nb, H, Lmax, device=dev())
        with pytest.raises(UiaError, match="cu_seqlens"):
            ops.attn_fwd(q, k, v, out, nb, H, Lmax, lse=lse, cu_seqlens=cu)
        with pytest.raises(UiaError, match="cu_seqlens"):
            ops.attn_fwd(q, k, v, out, nb, H, Lmax, mask="keypad", keylen=kl, cu_seqlens=cu)
    assert not bad, bad
    finish(chk)


# ---------------------------------------------------------------- g. small-head path

# the longest head each small-head launch accepts: 1024 tokens (the kernel's own cap) for head dim 16; for head dim 32 the K / V image in
# LDS, 2·L·dh·4 bytes forward (640) and (2·L·dh + 2·L)·4 bytes backward (620), of 160 KiB
SMALL_MAX = {(16, False): 1024, (16, True): 1024, (32, False): 640, (32, True): 620}


@pytest.mark.parametrize("dh", (16, 32))
def test_small_head(ops, UiaError, dh):
    """Head dim 16 / 32 (the CLIPSeg decoder): bf16 dh 16 unmasked up to 512 tokens runs the MFMA kernels, everything else the scalar
    ones.  Every length up to the pinned limit matches the reference; one token more is refused with UiaError."""
    chk, bad = R.Checker(), []
    fmax, bmax = SMALL_MAX[(dh, False)], SMALL_MAX[(dh, True)]
    for dt in DT:
        for L in sorted({1, 16, 17, 197, 485, 512, 513, bmax, fmax}):
            qkv, dout = fused(L, dt, dh, seed=11), dout_for(L, dt, dh)
            for mask in MASKS:
                kl = keylens(L) if mask == "keypad" else None
                ctx = f"small dh={dh} L={L} mask={mask}"
                out, lse = run_fwd(ops, qkv, L, dt, mask, kl, dh)
                ref = ref_of(qkv, L, mask, kl, dh, dout=dout)
                check_fwd(chk, out, lse, ref, L, dt, ctx, dh, tag=f" dh{dh}")
                if L <= bmax:
                    check_bwd(chk, run_bwd(ops, qkv, out, dout, lse, L, dt, mask, kl, dh), ref, L, dt, ctx, dh, tag=f" dh{dh}")
        for L, is_bwd in ((fmax + 1, False), (bmax + 1, True)):
            qkv, dout = fused(L, dt, dh, seed=12), dout_for(L, dt, dh)
            q, k, v = split(qkv, dh)
            out = torch.zeros(B * L, H * dh, device=dev(), dtype=dt)
            lse = torch.zeros(B, H, L, device=dev())
            d = torch.zeros(B * L, 3 * H * dh, device=dev(), dtype=dt)
            try:
                if is_bwd:
                    ops.attn_bwd(q, k, v, out, dout, lse, d[:, :H * dh], d[:, H * dh:2 * H * dh], d[:, 2 * H * dh:], B, H, L, dh=dh)
                else:
                    ops.attn_fwd(q, k, v, out, B, H, L, lse=lse, dh=dh)
                bad.append(f"dh={dh} {dt} {'bwd' if is_bwd else 'fwd'} L={L}: accepted past the limit")
            except UiaError:
                pass
    assert not bad, bad
    finish(chk)


# ---------------------------------------------------------------- h. argument contract

def test_argument_contract(ops, UiaError):
    """Bad shapes are refused with UiaError before any launch.  Every buffer is valid for the memory it describes."""
    from uia_hip.ops import KBlocked
    bf = torch.bfloat16

    def fwd_args(L, dh=64, dt=bf):
        qkv = torch.zeros(B * L, 3 * H * dh, device=dev(), dtype=dt)
        q, k, v = split(qkv, dh)
        return q, k, v, torch.zeros(B * L, H * dh, device=dev(), dtype=dt), torch.zeros(B, H, L, device=dev())

    q, k, v, out, lse = fwd_args(273)
    with pytest.raises(UiaError, match="L=273"):
        ops.attn_fwd(q, k, v, out, B, H, 273, lse=lse)
    for dt, L in ((bf, 289), (torch.float32, 273)):
        q, k, v, out, lse = fwd_args(L, dt=dt)
        d = torch.zeros(B * L, 3 * H * 64, device=dev(), dtype=dt)
        with pytest.raises(UiaError, match=f"L={L}"):
            ops.attn_bwd(q, k, v, out, out, lse, d[:, :128], d[:, 128:256], d[:, 256:], B, H, L)
    q, k, v, out, lse = fwd_args(17, dh=48)
    with pytest.raises(UiaError, match="head dim 48"):
        ops.attn_fwd(q, k, v, out, B, H, 17, lse=lse)
    for dh in (64, 32, 16):
        q, k, v, out, lse = fwd_args(17, dh=dh)
        with pytest.raises(UiaError, match="keylen"):
            ops.attn_fwd(q, k, v, out, B, H, 17, lse=lse, mask="keypad", dh=dh)
        d = torch.zeros(B * 17, 3 * H * dh, device=dev(), dtype=bf)
        D = H * dh
        with pytest.raises(UiaError, match="keylen"):
            ops.attn_bwd(q, k, v, out, out, lse, d[:, :D], d[:, D:2 * D], d[:, 2 * D:], B, H, 17, mask="keypad", dh=dh)
    q, k, v, out, lse = fwd_args(17, dh=32)
    kb = KBlocked(torch.zeros(H * 32 // 32, B * 17, 32, device=dev(), dtype=bf))
    with pytest.raises(UiaError, match="head dim 64"):
        ops.attn_fwd(q, k, v, kb, B, H, 17, lse=lse)
