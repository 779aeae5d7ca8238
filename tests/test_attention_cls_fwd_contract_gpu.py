"""ops.attn_fwd_cls (uia_attn_fwd_cls, csrc/cls_grad.hip) against the float64 reference of tests/attn_reference.py: the attention forward of the ONE query row
token 0 of every (sequence, head).  Same helpers and bars as test_attention_contract_gpu.py for one forward row (R.fwd, R.out_bound, R.lse_bound, R.Checker).
q / k / v are slices of a fused qkv tensor; out [B, H·64] and lse [B, H] are views inside NaN-filled buffers with guard elements behind them (guarded_out.Out),
so an element the kernel leaves unwritten, or a write outside the B rows, fails.  Under key padding the K and V rows at or beyond keylen hold NaN in what the
kernel reads (zeros in what the reference reads): a kernel that touched one would return NaN."""
import ctypes as C
import math

import pytest
import torch

import attn_reference as R
from guarded_out import Out

pytestmark = pytest.mark.gpu

DH = 64
LENGTHS = (1, 2, 16, 17, 32, 33, 197, 256, 257, 288)     # one token, the 32-key pass +- 1, the two tower lengths and their neighbours, the longest
SHAPES = ((1, 1), (3, 2), (2, 12))
DT = (torch.bfloat16, torch.float32)


def dev():
    return torch.device("cuda:0")


def keylens(L):
    """The five lengths the issue names: all padding (clamped to one key), one key, all but one, all, a little over half."""
    return (0, 1, L - 1, L, (L + 1) // 2 + 1)


def problem(B, H, L, dt, keylen=None):
    """(qkv the kernel reads, float64 reference of row 0).  With keylen, the K and V rows the mask hides are NaN for the kernel and zero for the reference."""
    D = H * DH
    g = torch.Generator(device=dev()).manual_seed(9000 + 97 * L + 7 * B + H)
    qkv = (torch.randn(B * L, 3 * D, device=dev(), generator=g) * 1.5).to(dt)
    clean = qkv.clone()
    if keylen is not None:
        n = R.clamp_keylen(keylen, L)
        hidden = (torch.arange(L, device=dev())[None, :] >= n.to(dev())[:, None]).reshape(B * L)
        qkv[hidden, D:] = float("nan")
        clean[hidden, D:] = 0
    q, k, v = (R.heads(t, B, L, H, DH) for t in (clean[:, :D], clean[:, D:2 * D], clean[:, 2 * D:]))
    f = R.fwd(q, k, v, "keypad" if keylen is not None else "none", keylen)
    return qkv, {key: f[key][:, :, :1] for key in ("out", "lse", "pabsv")}


def run_and_judge(chk, B, H, L, dt, keylen, ctx):
    from uia_hip import ops
    D = H * DH
    qkv, ref = problem(B, H, L, dt, keylen)
    out, lse = Out((B, D), dt), Out((B, H), torch.float32)
    kl = None if keylen is None else keylen.to(dev(), torch.int32).contiguous()
    ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out.t, B, H, L, lse=lse.t, mask=None if kl is None else "keypad", keylen=kl)
    torch.cuda.synchronize()
    got = out.t.reshape(B, 1, H, DH).permute(0, 2, 1, 3)                       # [B, H, 1, dh]
    chk.check(f"out {dt}", got, ref["out"], R.out_bound(ref["out"], ref["pabsv"], dt), ctx)
    chk.check(f"lse {dt}", lse.t.reshape(B, H, 1), ref["lse"], R.lse_bound(ref["lse"], dt), ctx)
    assert out.intact() and lse.intact(), f"{ctx}: a write outside out / lse"
    return qkv, out, lse


@pytest.mark.parametrize("dt", DT, ids=("bf16", "fp32"))
def test_cls_query_forward_against_float64_at_every_length_shape_and_mask(dt):
    chk = R.Checker()
    for L in LENGTHS:
        for B, H in SHAPES:
            run_and_judge(chk, B, H, L, dt, None, f"L={L} B={B} H={H} none")
            vals = keylens(L)
            for start in range(0, len(vals), B):                                # every length, mixed within the batch
                kl = torch.tensor([vals[(start + i) % len(vals)] for i in range(B)])
                run_and_judge(chk, B, H, L, dt, kl, f"L={L} B={B} H={H} keylen={kl.tolist()}")
    print("\n" + chk.report(0))
    assert chk.ok(), chk.report()


def test_two_launches_give_the_same_bits_and_lse_is_optional():
    from uia_hip import ops
    B, H, L, dt = 3, 2, 197, torch.bfloat16
    D = H * DH
    qkv, _ = problem(B, H, L, dt)
    a, b = Out((B, D), dt), Out((B, D), dt)
    la = Out((B, H), torch.float32)
    ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], a.t, B, H, L, lse=la.t)
    ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], b.t, B, H, L)
    torch.cuda.synchronize()
    assert torch.equal(a.t, b.t) and bool(torch.isfinite(a.t.float()).all()) and a.intact() and b.intact() and la.intact()


def test_the_backward_takes_the_compact_out_and_lse_the_forward_left():
    """uia_attn_bwd_cls_rows on (out [B, H·64], lse [B, H]) gives the bits uia_attn_bwd_cls gives on the dense tensors that hold the same rows at token 0."""
    from uia_hip import ops
    for dt in DT:
        B, H, L = 3, 2, 33
        D = H * DH
        qkv, _ = problem(B, H, L, dt)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        out = torch.empty(B, D, device=dev(), dtype=dt)
        lse = torch.empty(B, H, device=dev(), dtype=torch.float32)
        ops.attn_fwd_cls(q, k, v, out, B, H, L, lse=lse)
        dense_out = torch.zeros(B * L, D, device=dev(), dtype=dt)
        dense_out[::L] = out
        dense_lse = torch.zeros(B, H, L, device=dev(), dtype=torch.float32)
        dense_lse[:, :, 0] = lse
        g = torch.Generator(device=dev()).manual_seed(3)
        dout = torch.randn(B, D, device=dev(), generator=g).to(dt)
        d0 = torch.full((B * L, 3 * D), float("nan"), device=dev(), dtype=dt)
        d1 = torch.full((B * L, 3 * D), float("nan"), device=dev(), dtype=dt)
        ops.attn_bwd_cls(q, k, v, dense_out, dout, dense_lse, d0[:, :D], d0[:, D:2 * D], d0[:, 2 * D:], B, H, L)
        ops.attn_bwd_cls(q, k, v, out, dout, lse, d1[:, :D], d1[:, D:2 * D], d1[:, 2 * D:], B, H, L, rows=True)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(d1.float()).all()) and torch.equal(d0, d1), dt


def test_every_refused_argument_class_returns_its_error_code_without_a_launch():
    from uia_hip import _lib, ops
    B, H, L, dt = 3, 2, 16, torch.bfloat16
    D = H * DH
    qkv, _ = problem(B, H, L, dt)
    out = torch.full((B, D), float("nan"), device=dev(), dtype=dt)
    lse = torch.full((B, H), float("nan"), device=dev(), dtype=torch.float32)
    kl = torch.full((B,), L, device=dev(), dtype=torch.int32)
    lib = _lib.lib()

    def desc():
        return ops._attn_desc(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, lse, B, H, L, None, None, None)

    def refused(change, word, code=_lib.BF16):
        d = desc()
        change(d)
        rc = lib.uia_attn_fwd_cls(None, code, C.byref(d))
        msg = lib.uia_last_error()
        assert rc != 0 and word in msg, (rc, msg, word)

    def setter(**kw):
        def f(d):
            for k_, v_ in kw.items():
                setattr(d, k_, v_)
        return f
    assert lib.uia_attn_fwd_cls(None, _lib.BF16, None) != 0 and b"null descriptor" in lib.uia_last_error()
    refused(setter(), b"bad dtype", code=77)
    refused(setter(L=289), b"L=289")
    refused(setter(L=0), b"L=0")
    refused(setter(B=0), b"B=0")
    refused(setter(dh=32), b"head dim 32")
    refused(setter(mask_kind=1), b"mask kind 1")                                      # causal
    refused(setter(mask_kind=2), b"mask kind 2")                                      # key padding without key lengths
    refused(setter(keylen=kl.data_ptr()), b"mask kind 0")                             # key lengths without the mask kind
    refused(setter(cu_seqlens=kl.data_ptr()), b"packed")
    refused(setter(scale=0.0), b"scale")
    refused(setter(scale=float("inf")), b"scale")
    refused(setter(q=None), b"null tensor")
    refused(setter(out=None), b"null tensor")
    refused(setter(out_kb_rows=B * L), b"K-blocked")
    refused(setter(ldo=D - 8), b"leading dimension")
    refused(setter(ld_qkv=D - 8), b"leading dimension")
    refused(setter(ld_qkv=3 * D + 4), b"16-byte")
    refused(setter(ldo=D + 4), b"16-byte")
    refused(setter(k=qkv.data_ptr() + 2 * D + 2), b"alignment")
    refused(setter(out=out.data_ptr() + 2), b"alignment")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all())      # nothing was launched
    # the Python wrapper refuses what it can see before the library does
    with pytest.raises(_lib.UiaError, match="mask"):
        ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, B, H, L, mask="causal")
    with pytest.raises(_lib.UiaError, match="keylen"):
        ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, B, H, L, mask="keypad")
    with pytest.raises(_lib.UiaError, match="out must be"):
        ops.attn_fwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], torch.empty(B * L, D, device=dev(), dtype=dt), B, H, L)
    assert math.isnan(float(out[0, 0]))
