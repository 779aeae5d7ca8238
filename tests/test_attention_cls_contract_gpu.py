"""ops.attn_bwd_cls (uia_attn_bwd_cls, csrc/cls_grad.hip) against the float64 reference of tests/attn_reference.py: the attention backward for a dout that is zero
outside token 0 of every sequence.  Same helpers and bars as test_attention_contract_gpu.py (R.bwd, R.grad_bound, R.Checker); the destination is NaN-filled, so an
element the kernel leaves unwritten fails; both output layouts, `out` in both input layouts; dq rows l > 0 exactly zero; masks are refused."""
import pytest
import torch

import attn_reference as R

pytestmark = pytest.mark.gpu

B, H, DH = 3, 2, 64
D = H * DH
LENGTHS = (1, 2, 16, 17, 197, 257, 288)     # a single token, one tile +- 1, the two tower lengths, the dense kernel's longest
DT = (torch.bfloat16, torch.float32)


def dev():
    return torch.device("cuda:0")


def to_kb(rows_t):
    """[rows, cols] -> ops.KBlocked [cols / 32, rows, 32] (bf16)."""
    from uia_hip.ops import KBlocked
    rows, cols = rows_t.shape
    return KBlocked(rows_t.reshape(rows, cols // 32, 32).permute(1, 0, 2).contiguous())


def from_kb(kb):
    return kb.t.permute(1, 0, 2).reshape(kb.rows, kb.cols)


def problem(L, dt):
    """Operands as the kernel sees them (rounded to dt) and the float64 reference with dout zero outside token 0; out and lse are the reference's, rounded."""
    g = torch.Generator(device=dev()).manual_seed(7000 + L)
    qkv = (torch.randn(B * L, 3 * D, device=dev(), generator=g) * 1.5).to(dt)
    do_cls = torch.randn(B, D, device=dev(), generator=g).to(dt)
    dout = torch.zeros(B * L, D, device=dev(), dtype=dt)
    dout[::L] = do_cls
    q, k, v = (R.heads(t, B, L, H, DH) for t in (qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]))
    f = R.fwd(q, k, v)
    out = R.rows(f["out"]).to(dt)
    lse = f["lse"].to(torch.float32).contiguous()
    ref = R.bwd(q, k, v, R.heads(dout, B, L, H, DH))
    return qkv, do_cls, out, lse, ref


def judge(chk, grads, ref, L, dt, ctx):
    for name, g in zip(("dq", "dk", "dv"), grads):
        chk.check(f"{name} {dt}", R.heads(g, B, L, H, DH), ref[name], R.grad_bound(ref[name], ref["mag_" + name], dt), ctx)
    dq = grads[0].reshape(B, L, D)
    assert bool((dq[:, 1:] == 0).all()), f"{ctx}: dq rows l > 0 must be exactly zero"


@pytest.mark.parametrize("dt", DT, ids=("bf16", "fp32"))
def test_cls_query_backward_against_float64_at_every_length_and_layout(dt):
    from uia_hip import ops
    chk = R.Checker()
    for L in LENGTHS:
        qkv, do_cls, out, lse, ref = problem(L, dt)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        outs = [("rows", out)] + ([("kb", to_kb(out))] if dt == torch.bfloat16 else [])
        for oname, o in outs:
            d = torch.full((B * L, 3 * D), float("nan"), device=dev(), dtype=dt)
            ops.attn_bwd_cls(q, k, v, o, do_cls, lse, d[:, :D], d[:, D:2 * D], d[:, 2 * D:], B, H, L)
            judge(chk, (d[:, :D], d[:, D:2 * D], d[:, 2 * D:]), ref, L, dt, f"L={L} out={oname} dqkv=rows")
            if dt == torch.bfloat16:
                dkb = to_kb(torch.full((B * L, 3 * D), float("nan"), device=dev(), dtype=dt))
                ops.attn_bwd_cls(q, k, v, o, do_cls, lse, dkb, None, None, B, H, L)
                r = from_kb(dkb)
                judge(chk, (r[:, :D], r[:, D:2 * D], r[:, 2 * D:]), ref, L, dt, f"L={L} out={oname} dqkv=kb")
                assert torch.equal(r, d), f"L={L} out={oname}: the K-blocked result differs from the row-major one"
    print("\n" + chk.report(0))
    assert chk.ok(), chk.report()


def test_k_blocked_destination_inside_a_larger_tensor_leaves_the_other_rows_alone():
    """dqkv_kb_rows is the plane stride of the WHOLE K-blocked tensor: rows past B*L keep what they held."""
    from uia_hip import ops
    L, dt = 17, torch.bfloat16
    qkv, do_cls, out, lse, ref = problem(L, dt)
    whole = ops.KBlocked(torch.full((3 * D // 32, B * L + 5, 32), 3.0, device=dev(), dtype=dt))
    ops.attn_bwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, do_cls, lse, whole.row_range(0, B * L), None, None, B, H, L)
    assert bool((whole.t[:, B * L:] == 3.0).all())
    chk = R.Checker()
    r = whole.t[:, :B * L].permute(1, 0, 2).reshape(B * L, 3 * D)
    judge(chk, (r[:, :D], r[:, D:2 * D], r[:, 2 * D:]), ref, L, dt, "L=17 row range")
    assert chk.ok(), chk.report()


@pytest.mark.parametrize("mask", ("causal", "keypad"))
def test_masks_are_refused(mask):
    from uia_hip import ops
    from uia_hip._lib import UiaError
    L, dt = 16, torch.bfloat16
    qkv, do_cls, out, lse, _ = problem(L, dt)
    d = torch.zeros(B * L, 3 * D, device=dev(), dtype=dt)
    with pytest.raises(UiaError, match="mask"):
        ops.attn_bwd_cls(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, do_cls, lse, d[:, :D], d[:, D:2 * D], d[:, 2 * D:], B, H, L, mask=mask)


def test_the_c_entry_point_refuses_a_mask_kind_and_a_long_sequence():
    import ctypes as C
    from uia_hip import _lib, ops
    L, dt = 16, torch.bfloat16
    qkv, do_cls, out, lse, _ = problem(L, dt)
    d = torch.zeros(B * L, 3 * D, device=dev(), dtype=dt)
    desc = ops._attn_desc(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out, lse, B, H, L, "causal", None, None)
    desc.dout, desc.lddo = do_cls.data_ptr(), D
    desc.dq, desc.dk, desc.dv, desc.ld_dqkv = d.data_ptr(), d.data_ptr() + 2 * D, d.data_ptr() + 4 * D, 3 * D
    assert _lib.lib().uia_attn_bwd_cls(None, _lib.BF16, C.byref(desc)) != 0 and b"mask" in _lib.lib().uia_last_error()
    desc.mask_kind, desc.L = 0, 289
    assert _lib.lib().uia_attn_bwd_cls(None, _lib.BF16, C.byref(desc)) != 0 and b"L=289" in _lib.lib().uia_last_error()
