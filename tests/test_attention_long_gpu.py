"""-m gpu: ops.attn_fwd_long (uia_attn_fwd_long), the online-softmax forward for sequences of any length, judged element-wise against
the float64 reference of tests/attn_reference.py on the operands the kernel sees, under the bars of test_forward_length_sweep.

Why the single-pass bars hold for the online form.  Block n of the key sweep exponentiates its scores against the running max m_n
(exp2 of an fp32 fma, as the single-pass kernel does against the final max) and, in bf16, rounds those weights once for the P·V
product: each term P_ij·v_j is carried with one bf16 rounding of P_ij, exactly as before.  What is new is the rescale
O ← α·O, l ← α·l with α = exp2((m_old − m_new)·scale) when a later block raises the max.  α is exactly 1 when the max does not
grow, and each growth is one fp32 multiply (2^-24 relative) applied to O and l alike, so their ratio moves by at most 2·k·2^-24
after k growths.  For the bf16 bar (C·2^-8·P·|V|, C = 2.2) that is invisible at any k below 10^4.  For the fp32 bar
(290·2^-24·P·|V|) the kernel rescales per 16-key chunk; random scores raise the max in O(log n) chunks, and the test below that
raises it in EVERY chunk (k = L/16 = 64 at L = 1024) stays under C_OUT_OFFSET's 900 for fp32, the bar of shifted score rows in
the single-pass contract.  So no new constant is introduced."""

import pytest
import torch

import attn_reference as R

pytestmark = pytest.mark.gpu

H = 2
DT = (torch.bfloat16, torch.float32)
LENGTHS = (1, 16, 17, 64, 65, 272, 273, 288, 289, 511, 512, 513, 577, 1024, 1369, 1370, 1371, 2048, 4100)


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


def nb(L):
    """Batch rows per length: the float64 reference holds B·H·L² probabilities."""
    return 3 if L <= 1024 else (2 if L <= 2048 else 1)


def fused(L, dt, B, seed=0):
    g = torch.Generator(device=dev()).manual_seed(seed * 1000 + L)
    return (torch.randn(B * L, 3 * H * 64, device=dev(), generator=g) * 1.5).to(dt)


def split(qkv):
    D = H * 64
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]


def run(ops, qkv, L, B, dt, scale=None):
    q, k, v = split(qkv)
    out = torch.full((B * L, H * 64), float("nan"), device=dev(), dtype=dt)
    lse = torch.full((B, H, L), float("nan"), device=dev())
    ops.attn_fwd_long(q, k, v, out, B, H, L, lse=lse, scale=scale)
    return out, lse


def ref_of(qkv, L, B, scale=None):
    q, k, v = (R.heads(t, B, L, H, 64) for t in split(qkv))
    return R.fwd(q, k, v, "none", None, scale)


def check(chk, out, lse, ref, L, B, dt, ctx, c_out=None):
    o = R.heads(out, B, L, H, 64)
    chk.check(f"out {dt}", o, ref["out"], R.out_bound(ref["out"], ref["pabsv"], dt, c_out), ctx)
    if lse is not None:
        chk.check(f"lse {dt}", lse, ref["lse"], R.lse_bound(ref["lse"], dt), ctx)


def finish(chk):
    print("\n" + chk.report(0))
    assert chk.ok(), chk.report()


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("dt", DT)
def test_long_length_sweep(ops, dt):
    chk = R.Checker()
    for L in LENGTHS:
        B = nb(L)
        qkv = fused(L, dt, B)
        out, lse = run(ops, qkv, L, B, dt)
        check(chk, out, lse, ref_of(qkv, L, B), L, B, dt, f"long L={L}")
        del qkv, out, lse
        torch.cuda.empty_cache()
    finish(chk)


@pytest.mark.parametrize("dt", DT)
def test_long_structured_exact(ops, dt):
    """K = 0: every score is equal, out is the mean of the V rows to one rounding, lse = log L."""
    chk = R.Checker()
    for L in (1, 65, 273, 1370, 4100):
        B = nb(L)
        v = R.structured_v(B, H, L, 64, dev())
        qkv = fused(L, dt, B, seed=3)
        qkv[:, H * 64:2 * H * 64] = 0
        qkv[:, 2 * H * 64:] = R.rows(v).to(dt)
        out, lse = run(ops, qkv, L, B, dt)
        o_ref, lse_ref = R.closed_fwd(R.heads(qkv[:, 2 * H * 64:], B, L, H, 64), "none")
        chk.check(f"out exact {dt}", R.heads(out, B, L, H, 64), o_ref, R.one_rounding_bound(o_ref, dt), f"structured L={L}")
        chk.check(f"lse exact {dt}", lse, lse_ref, R.lse_exact_bound(lse_ref), f"structured L={L}")
    finish(chk)


def offset_case(L, B, dt, where, seed):
    """Scores of moderate spread plus a large offset on chosen keys: `first` puts each row's maximum in the first key block, `last` in
    the last one, `rising` adds an offset that grows with the key index, so the running max grows in every block (and every fp32 chunk)."""
    g = torch.Generator(device=dev()).manual_seed(seed * 7919 + L)
    qkv = torch.randn(B * L, 3 * H * 64, device=dev(), generator=g)
    D = H * 64
    q = qkv[:, :D].view(B * L, H, 64)
    q[..., 0] = 4.0                                      # a fixed component: the score of key j gains 4·k_j[0]·scale
    k = qkv[:, D:2 * D].view(B, L, H, 64)
    j = torch.arange(L, device=dev(), dtype=torch.float32)
    if where == "first":
        k[:, :min(L, 64), :, 0] += 20.0
    elif where == "last":
        k[:, max(0, L - 1 - (L - 1) % 64):, :, 0] += 20.0
    else:
        k[:, :, :, 0] += (j * (40.0 / max(L, 1)))[None, :, None]
    return qkv.to(dt)


@pytest.mark.parametrize("dt", DT)
def test_long_score_offsets(ops, dt):
    chk = R.Checker()
    for L in (273, 577, 1024, 1370):
        B = 2
        for i, where in enumerate(("first", "last", "rising")):
            qkv = offset_case(L, B, dt, where, seed=i + 1)
            out, lse = run(ops, qkv, L, B, dt)
            check(chk, out, lse, ref_of(qkv, L, B), L, B, dt, f"offset {where} L={L}", c_out=R.C_OUT_OFFSET[dt])
        for scale in (0.03, 0.37):
            qkv = fused(L, dt, B, seed=6)
            out, lse = run(ops, qkv, L, B, dt, scale=scale)
            check(chk, out, lse, ref_of(qkv, L, B, scale=scale), L, B, dt, f"scale={scale} L={L}")
    finish(chk)


G = 3


def sentinel(shape, dt):
    t = torch.empty(shape, device=dev(), dtype=dt)
    bits(t).fill_(0x7FC5 if dt == torch.bfloat16 else 0x7FC00005)
    return t


@pytest.mark.parametrize("dt", DT)
def test_long_writes_stay_inside(ops, dt):
    """out and lse in sentinel buffers with guard rows and a row pitch wider than H·64; q / k / v as strided slices of a wider fused
    buffer whose spare columns hold NaN (a read outside the head's columns would poison the result)."""
    chk, bad = R.Checker(), []
    pad = 8 if dt == torch.bfloat16 else 4
    D = H * 64
    for L in (1, 17, 273, 577, 1370):
        B = nb(L)
        base = fused(L, dt, B, seed=8)
        wide = torch.full((B * L, 3 * (D + pad)), float("nan"), device=dev(), dtype=dt)
        for i in range(3):
            wide[:, i * (D + pad):i * (D + pad) + D] = base[:, i * D:(i + 1) * D]
        q, k, v = (wide[:, i * (D + pad):i * (D + pad) + D] for i in range(3))
        obuf = sentinel((B * L + 2 * G, D + pad), dt)
        out = obuf[G:G + B * L, :D]
        lbuf = sentinel((B * H * L + 2 * G,), torch.float32)
        lse = lbuf[G:G + B * H * L].view(B, H, L)
        ops.attn_fwd_long(q, k, v, out, B, H, L, lse=lse)
        check(chk, out, lse, ref_of(base, L, B), L, B, dt, f"guarded L={L}")
        mask = torch.ones(obuf.shape, dtype=torch.bool, device=dev())
        mask[G:G + B * L, :D] = False
        if not torch.equal(bits(obuf[mask]), bits(sentinel(obuf[mask].shape, dt))):
            bad.append(f"L={L}: wrote outside out")
        if not (torch.equal(bits(lbuf[:G]), bits(sentinel((G,), torch.float32))) and torch.equal(bits(lbuf[-G:]), bits(sentinel((G,), torch.float32)))):
            bad.append(f"L={L}: wrote outside lse")
    assert not bad, bad
    finish(chk)


@pytest.mark.parametrize("dt", DT)
def test_long_deterministic(ops, dt):
    for L in (577, 1370):
        qkv = fused(L, dt, 2, seed=9)
        o1, l1 = run(ops, qkv, L, 2, dt)
        o2, l2 = run(ops, qkv, L, 2, dt)
        assert torch.equal(bits(o1), bits(o2)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32)), f"L={L}: two runs differ"


@pytest.mark.parametrize("dt", DT)
def test_long_agrees_with_single_pass(ops, dt):
    """For L <= 272 both forwards are held to the reference's bars, and to each other within the sum of those bars."""
    chk = R.Checker()
    for L in (1, 16, 17, 64, 65, 197, 257, 272):
        B = 3
        qkv = fused(L, dt, B, seed=4)
        q, k, v = split(qkv)
        o1 = torch.full((B * L, H * 64), float("nan"), device=dev(), dtype=dt)
        l1 = torch.empty(B, H, L, device=dev())
        ops.attn_fwd(q, k, v, o1, B, H, L, lse=l1)
        o2, l2 = run(ops, qkv, L, B, dt)
        ref = ref_of(qkv, L, B)
        bound = R.out_bound(ref["out"], ref["pabsv"], dt)
        chk.check(f"long vs single-pass out {dt}", R.heads(o2, B, L, H, 64).double(), R.heads(o1, B, L, H, 64).double(), 2 * bound, f"agree L={L}")
        chk.check(f"long vs single-pass lse {dt}", l2.double(), l1.double(), 2 * R.lse_bound(ref["lse"], dt), f"agree L={L}")
        check(chk, o2, l2, ref, L, B, dt, f"agree L={L}")
    finish(chk)


def test_long_argument_contract(ops, UiaError):
    """uia_attn_fwd_long refuses what it cannot compute before any launch; uia_attn_fwd keeps its 272-token limit."""
    import ctypes as C
    from uia_hip import _lib
    dt = torch.bfloat16
    L, B = 300, 1
    qkv = fused(L, dt, B)
    q, k, v = split(qkv)
    out = torch.zeros(B * L, H * 64, device=dev(), dtype=dt)

    def refused(fn):
        try:
            fn()
        except UiaError:
            return True
        return False

    def raw(**kw):
        d = ops._attn_desc(q, k, v, out, None, B, H, L, None, None, None)
        for name, val in kw.items():
            setattr(d, name, val)
        return _lib.lib().uia_attn_fwd_long(None, ops._code(dt), C.byref(d))

    assert raw() == 0
    torch.cuda.synchronize()
    cases = {
        "dh 32": dict(dh=32),
        "causal mask": dict(mask_kind=1),
        "keypad mask": dict(mask_kind=2),
        "cu_seqlens": dict(cu_seqlens=q.data_ptr()),
        "K-blocked out": dict(out_kb_rows=B * L),
        "null q": dict(q=None),
        "null out": dict(out=None),
        "misaligned q": dict(q=q.data_ptr() + 2),
        "misaligned out": dict(out=out.data_ptr() + 4),
        "ld_qkv not 16-byte": dict(ld_qkv=3 * H * 64 + 1),
        "ldo not 16-byte": dict(ldo=H * 64 + 4),
        "L = 0": dict(L=0),
        "scale 0": dict(scale=0.0),
    }
    accepted = [name for name, kw in cases.items() if raw(**kw) == 0]
    assert not accepted, f"accepted: {accepted}"
    assert b"uia_attn_fwd_long" in _lib.lib().uia_last_error()
    with pytest.raises(UiaError):
        ops.attn_fwd_long(q[:, :64], k[:, :64], v[:, :64], out[:, :64], B, 2, L)        # head dim 32
    with pytest.raises(UiaError):
        ops.attn_fwd(q, k, v, out, B, H, 273 if L >= 273 else L)                       # the single-pass forward still stops at 272
