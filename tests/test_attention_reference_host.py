"""Host-only checks of tests/attn_reference.py (no GPU): the float64 reference against torch's SDPA and autograd, its closed forms
for K = 0 against the reference, and the sensitivity of the bounds: the reference's own output with a planted bug must trip the
bars the GPU contract tests apply to the kernels (tests/test_attention_contract_gpu.py), at every swept length."""
import math

import pytest
import torch

import attn_reference as R

B, H = 3, 2
MASKS = ("none", "causal", "keypad")
SWEEP = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 80, 81, 128, 129, 208, 209, 240, 241, 256, 257, 272, 288)


def keylens(L):
    ch = (1, 15, 16, 17, L - 1, L, L + 5)
    return torch.tensor([ch[(L + 3 * b) % 7] for b in range(B)], dtype=torch.int32)


def operands(L, dh=64, dt=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + L)
    return [(torch.randn(B, H, L, dh, generator=g) * 1.5).to(dt).to(R.F64) for _ in range(4)]


@pytest.mark.parametrize("dh", (16, 32, 64))
@pytest.mark.parametrize("mask", MASKS)
def test_reference_matches_sdpa_and_autograd(mask, dh):
    for L in (1, 17, 80, 129):
        q, k, v, do = operands(L, dh)
        kl = keylens(L) if mask == "keypad" else None
        for scale in (None, 0.37):
            ref = R.bwd(q, k, v, do, mask, kl, scale)
            qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
            o = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, attn_mask=R.visible(B, L, mask, kl), scale=R.kernel_scale(scale, dh))
            o.backward(do)
            s = (q @ k.transpose(-1, -2) * R.kernel_scale(scale, dh)).masked_fill(~R.visible(B, L, mask, kl), -math.inf)
            for got, want in ((ref["out"], o), (ref["lse"], torch.logsumexp(s, -1)), (ref["dq"], qq.grad), (ref["dk"], kk.grad), (ref["dv"], vv.grad)):
                assert torch.allclose(got, want.detach(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mask", MASKS)
def test_packed_reference_is_per_sequence(mask):
    lens = (1, 15, 16, 17, 77)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    x = torch.randn(cu[-1], 3 * H * 64, dtype=R.F64)
    q, k, v = x[:, :128], x[:, 128:256], x[:, 256:]
    out, _ = R.fwd_packed(q, k, v, cu, H, 64, mask if mask != "keypad" else "none")
    for b, n in enumerate(lens):
        f = R.fwd(*(R.heads(t[cu[b]:cu[b + 1]], 1, n, H, 64) for t in (q, k, v)), mask=mask if mask != "keypad" else "none")
        assert torch.equal(out[cu[b]:cu[b + 1]], R.rows(f["out"]))


@pytest.mark.parametrize("mask", MASKS)
def test_closed_forms_match_reference(mask):
    for L in SWEEP:
        q, _, _, do = operands(L)
        v = R.structured_v(B, H, L, 64)
        kl = keylens(L) if mask == "keypad" else None
        ref = R.bwd(q, torch.zeros_like(q), v, do, mask, kl)
        o, lse = R.closed_fwd(v, mask, kl)
        dq, dk, dv = R.closed_bwd(q, v, do, mask, kl)
        assert torch.allclose(o, ref["out"], rtol=1e-13, atol=1e-14) and torch.allclose(lse, ref["lse"], rtol=1e-13, atol=1e-14)
        assert torch.equal(dq, torch.zeros_like(dq)) and torch.allclose(ref["dq"], dq, atol=1e-12)
        assert torch.allclose(dk, ref["dk"], rtol=1e-10, atol=1e-11) and torch.allclose(dv, ref["dv"], rtol=1e-12, atol=1e-13)


# ---------------------------------------------------------------- sensitivity: planted bugs

def trunc_bf16(x):
    """Round toward zero to bf16 (the planted bug; torch's .to(bfloat16) rounds to nearest even)."""
    b = x.float().view(torch.int32) & ~0xFFFF
    return b.view(torch.float32).to(R.F64)


def buggy(bug, q, k, v, mask, kl):
    """(out, lse, stored) of the reference with `bug` planted; stored rounds out as the buggy kernel would."""
    B_, H_, L, dh = q.shape
    vis = R.visible(B_, L, mask, kl)
    j = torch.arange(L)
    rne = lambda o: o.to(torch.bfloat16).to(R.F64)  # noqa: E731
    if bug == "drop_last_key":                        # the last key each query sees
        last = (vis * j).amax(-1, keepdim=True)
        vis = vis & (j != last)
    elif bug == "causal_diag_excluded":
        vis = j[None, :] < j[:, None]
    elif bug.startswith("tile"):                       # one 16-key tile never multiplied
        t = int(bug[4:])
        vis = vis & ~((j >= 16 * t) & (j < 16 * t + 16))
    f = R.fwd(q, k, v, vis=vis.expand(B_, 1, L, L))
    out, lse = f["out"], f["lse"]
    if bug == "lse_shift":
        lse = lse + 2.0 ** -6
    if bug == "norm_n_plus_1":                         # a phantom key at the row max with V = 0: P normalised by (n + 1) for equal scores
        pm = f["p"].amax(-1)
        out, lse = out / (1 + pm)[..., None], lse + torch.log1p(pm)
    return out, lse, (trunc_bf16(out) if bug == "trunc" else rne(out))


def flagged(bug, L, mask, dt=torch.bfloat16):
    """Do the bars of the contract tests flag the planted bug on the random operands or on the structured ones?"""
    kl = keylens(L) if mask == "keypad" else None
    chk = R.Checker()
    q, k, v, _ = operands(L)
    ref = R.fwd(q, k, v, mask, kl)
    _, lse, stored = buggy(bug, q, k, v, mask, kl)
    chk.check("out", stored, ref["out"], R.out_bound(ref["out"], ref["pabsv"], dt), "random")
    chk.check("lse", lse.float(), ref["lse"], R.lse_bound(ref["lse"], dt), "random")
    vs = R.structured_v(B, H, L, 64)
    o_ref, lse_ref = R.closed_fwd(vs, mask, kl)
    _, lse, stored = buggy(bug, q, torch.zeros_like(k), vs, mask, kl)
    chk.check("out exact", stored, o_ref, R.one_rounding_bound(o_ref, dt), "structured")
    chk.check("lse exact", lse.float(), lse_ref, R.lse_exact_bound(lse_ref), "structured")
    return not chk.ok()


def trunc_is_noop(L, mask):
    """Truncation is caught by the one-rounding bar of the structured answers (the scale-aware random bar is wider than an ulp).
    Where every structured answer rounds the same either way (L <= 2; unmasked L = 16, 32, 64, 128, 256, where n is a power of two
    and every mean is exact, and 257 = 2^8 + 1, whose means carry eight zero bits past the bf16 mantissa) there is nothing to catch."""
    o, _ = R.closed_fwd(R.structured_v(B, H, L, 64), mask, keylens(L) if mask == "keypad" else None)
    return torch.equal(trunc_bf16(o), o.to(torch.bfloat16).to(R.F64))


@pytest.mark.parametrize("mask", MASKS)
def test_correct_answer_passes_every_bar(mask):
    for L in SWEEP:
        assert not flagged("none", L, mask), (L, mask)


@pytest.mark.parametrize("mask", MASKS)
def test_planted_bugs_are_caught(mask):
    missed = []
    for L in SWEEP:
        seen = int(R.clamp_keylen(keylens(L), L).max()) if mask == "keypad" else L      # keys any query sees: a tile past them is no bug
        bugs = ["drop_last_key", "lse_shift", "norm_n_plus_1"] + [f"tile{t}" for t in range((seen + 15) // 16)]
        if mask == "causal":
            bugs.append("causal_diag_excluded")
        if not trunc_is_noop(L, mask):
            bugs.append("trunc")
        missed += [f"{bug} L={L}" for bug in bugs if not flagged(bug, L, mask)]
    assert not missed, missed
    assert [L for L in SWEEP if trunc_is_noop(L, mask)] == {"none": [1, 2, 16, 32, 64, 128, 256, 257]}.get(mask, [1, 2])
