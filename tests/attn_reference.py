"""Float64 attention reference and the bounds that judge the HIP attention kernels against it.

A plain module, no pytest: tests/test_attention_contract_gpu.py runs it on the GPU next to ops.attn_fwd / ops.attn_bwd,
tests/test_attention_reference_host.py checks it (and shows that the bounds catch planted bugs) on the CPU.

Layout: the kernels read element (b, l, h, d) of q / k / v / out at row b*L + l, column h*dh + d.  The reference works on
[B, H, L, dh] float64 copies of exactly the operands the kernel sees (already rounded to bf16 / fp32), so the only
differences left are the kernel's own arithmetic.  Masks: "none", "causal" (query i sees keys j <= i), "keypad" (batch row b
sees keys j < keylen[b], keylen clamped to [1, L] as the kernels clamp it).  Packed sequences (cu_seqlens): sequence b is
rows cu[b] .. cu[b+1]-1, unmasked.
"""
import math

import torch

F64 = torch.float64

# ---- calibrated constants.  Each is about 2x the worst error-to-bound ratio measured on the MI355X with the constant set to 1, over
#      every comparison of test_attention_contract_gpu.py that uses it (measured worst in the comment; fp32 errors grow with |score|,
#      so the fp32 worst cases come from the scale = 0.37 runs, about 40 at the default scale)
C_OUT = {torch.bfloat16: 2.2, torch.float32: 290.0}       # out: |o - ref| <= C·u·(P·|V|) + u'·|ref|   measured 1.12 / 149
C_OUT_OFFSET = {torch.bfloat16: 1.9, torch.float32: 900.0}  # out with each row's scores moved by up to 80           measured 0.98 / 451
C_LSE = {torch.bfloat16: 1.1e-5, torch.float32: 3e-5}     # lse: |lse - ref| <= C (absolute, natural log)   measured 5.6e-6 / 1.5e-5
C_GRAD = {torch.bfloat16: 2.5, torch.float32: 330.0}      # dq / dk / dv: |g - ref| <= C·u·mag + u'·|ref|  measured 1.27 / 167

# u: the unit the C terms are counted in; u': the rounding of the stored result (the issue's form for bf16: 2^-8 and 2^-9)
_U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
_U_OUT = {torch.bfloat16: 2.0 ** -9, torch.float32: 2.0 ** -24}


def kernel_scale(scale, dh):
    """The softmax scale as the kernel holds it: an fp32 number."""
    s = dh ** -0.5 if scale is None else scale
    return float(torch.tensor(s, dtype=torch.float32))


def heads(x, B, L, H, dh):
    """[B*L, >= H*dh] rows (a view of fused qkv is fine) -> [B, H, L, dh] float64."""
    return x[:, :H * dh].reshape(B, L, H, dh).permute(0, 2, 1, 3).to(F64)


def rows(x):
    """[B, H, L, dh] -> [B*L, H*dh]."""
    B, H, L, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * dh)


def clamp_keylen(keylen, L):
    return keylen.to(torch.int64).clamp(1, L)


def visible(B, L, mask, keylen=None, device=None):
    """bool [B, 1, L, L]: query i (dim 2) sees key j (dim 3)."""
    j = torch.arange(L, device=device)
    if mask == "causal":
        return (j[None, :] <= j[:, None]).expand(B, 1, L, L)
    if mask == "keypad":
        kl = clamp_keylen(keylen, L).to(device)
        return (j[None, :] < kl[:, None])[:, None, None, :].expand(B, 1, L, L)
    assert mask in (None, "none"), mask
    return torch.ones(B, 1, L, L, dtype=torch.bool, device=device)


def fwd(q, k, v, mask="none", keylen=None, scale=None, vis=None):
    """q, k, v [B, H, L, dh] float64.  Returns dict(out, lse, p, pabsv): out [B,H,L,dh], lse [B,H,L], the probabilities
    p [B,H,L,L] and P·|V|, the scale of the bf16 forward bound."""
    B, H, L, dh = q.shape
    sc = kernel_scale(scale, dh)
    vis = visible(B, L, mask, keylen, q.device) if vis is None else vis
    s = (q @ k.transpose(-1, -2) * sc).masked_fill(~vis, -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    return dict(out=p @ v, lse=lse, p=p, pabsv=p @ v.abs())


def bwd(q, k, v, dout, mask="none", keylen=None, scale=None, vis=None):
    """Gradients of sum(out · dout) with respect to q, k, v (all [B, H, L, dh] float64), and the magnitudes the bounds scale with:
    mag_dq = s·A·|K|, mag_dk = s·Aᵀ·|Q|, mag_dv = Pᵀ·|dO| with A = P ⊙ (|dP| + |dO|·|O|) (the |dO|·|O| term covers δ = rowsum(dO ⊙ O)
    being formed from the kernel's own rounded O)."""
    f = fwd(q, k, v, mask, keylen, scale, vis)
    sc = kernel_scale(scale, q.shape[-1])
    p, o = f["p"], f["out"]
    dp = dout @ v.transpose(-1, -2)
    delta = (dout * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    a = p * (dp.abs() + (dout.abs() * o.abs()).sum(-1, keepdim=True))
    return dict(f, dq=sc * ds @ k, dk=sc * ds.transpose(-1, -2) @ q, dv=p.transpose(-1, -2) @ dout,
                mag_dq=sc * a @ k.abs(), mag_dk=sc * a.transpose(-1, -2) @ q.abs(), mag_dv=p.transpose(-1, -2) @ dout.abs())


def fwd_packed(q, k, v, cu, H, dh, mask="none", scale=None):
    """q, k, v [T, >= H*dh] rows of packed sequences; returns out [T, H*dh] float64 and pabsv likewise."""
    cu = [int(x) for x in cu]
    out = torch.zeros(cu[-1], H * dh, dtype=F64, device=q.device)
    pabsv = torch.zeros_like(out)
    for b in range(len(cu) - 1):
        lo, hi = cu[b], cu[b + 1]
        f = fwd(*(heads(t[lo:hi], 1, hi - lo, H, dh) for t in (q, k, v)), mask=mask, scale=scale)
        out[lo:hi], pabsv[lo:hi] = rows(f["out"]), rows(f["pabsv"])
    return out, pabsv


# ---- structured inputs with exact answers: K = 0 gives every visible key the weight 1/n; V[j, (j + h) mod dh] = w_j identifies key j

def key_weight(L, device=None):
    """w_j = 1 + (j mod 128)/128: exact in bf16, different for the keys that share a column below 128 apart."""
    return 1.0 + (torch.arange(L, device=device) % 128).to(F64) / 128.0


def structured_v(B, H, L, dh, device=None):
    v = torch.zeros(B, H, L, dh, dtype=F64, device=device)
    j = torch.arange(L, device=device)
    w = key_weight(L, device)
    for h in range(H):
        v[:, h, j, (j + h) % dh] = w
    return v


def counts(B, L, mask, keylen=None, device=None):
    """n [B, 1, L]: keys query i sees."""
    i = torch.arange(L, device=device, dtype=F64)
    if mask == "causal":
        return (i + 1).expand(B, 1, L)
    if mask == "keypad":
        return clamp_keylen(keylen, L).to(device).to(F64)[:, None, None].expand(B, 1, L)
    return torch.full((B, 1, L), float(L), dtype=F64, device=device)


def closed_fwd(v, mask, keylen=None):
    """out and lse of attention with K = 0, by prefix sums instead of a softmax: the mean of the visible V rows, lse = log n."""
    B, H, L, dh = v.shape
    n = counts(B, L, mask, keylen, v.device)
    if mask == "causal":
        num = v.cumsum(2)
    else:
        kl = clamp_keylen(keylen, L).tolist() if mask == "keypad" else [L] * B
        num = torch.stack([v[b, :, :kl[b]].sum(1, keepdim=True).expand(H, L, dh) for b in range(B)])
    return num / n[..., None], torch.log(n).expand(B, H, L)


def closed_bwd(q, v, dout, mask, keylen=None, scale=None):
    """dq, dk, dv of attention with K = 0.  P_ij = 1/n_i on visible keys, so dq = 0, dv_j = Σ_{i sees j} dO_i / n_i and
    dk_j = s·Σ_{i sees j} (dO_i·v_j − δ_i) q_i / n_i = s·(M_j v_j − r_j) with M_j = Σ_{i sees j} q_i dO_iᵀ / n_i, r_j = Σ_{i sees j} δ_i q_i / n_i."""
    B, H, L, dh = q.shape
    sc = kernel_scale(scale, dh)
    n = counts(B, L, mask, keylen, q.device)[..., None]               # [B, 1, L, 1]
    o, _ = closed_fwd(v, mask, keylen)
    delta = (dout * o).sum(-1, keepdim=True)
    g, qd, qr = dout / n, q[..., :, None] * dout[..., None, :] / n[..., None], q * delta / n
    if mask == "causal":                                              # the queries i >= j see key j: suffix sums
        dv, M, r = (t.flip(2).cumsum(2).flip(2) for t in (g, qd, qr))
    else:
        dv, M, r = (t.sum(2, keepdim=True).expand_as(t) for t in (g, qd, qr))
        if mask == "keypad":
            kl = clamp_keylen(keylen, L).to(q.device)
            seen = (torch.arange(L, device=q.device)[None, :] < kl[:, None])[:, None, :, None]
            dv, M, r = dv * seen, M * seen[..., None], r * seen
    dk = sc * ((M * v[..., None, :]).sum(-1) - r)
    return torch.zeros_like(q), dk, dv


# ---- bounds

def out_bound(ref, pabsv, dtype, c=None):
    c = C_OUT[dtype] if c is None else c
    return c * _U[dtype] * pabsv + _U_OUT[dtype] * ref.abs()


def grad_bound(ref, mag, dtype, c=None):
    c = C_GRAD[dtype] if c is None else c
    return c * _U[dtype] * mag + _U_OUT[dtype] * ref.abs()


def lse_bound(ref, dtype, c=None):
    return torch.full_like(ref, C_LSE[dtype] if c is None else c)


def one_rounding_bound(ref, dtype):
    """Half an ulp of the stored type at |ref| (the error of one round-to-nearest), plus fp32 slack for the 1/n product."""
    a = ref.abs()
    if dtype == torch.float32:
        return 2.0 ** -22 * a
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -126)))
    return torch.where(a > 0, torch.exp2(e - 8) + 2.0 ** -20 * a, torch.zeros_like(a))


def lse_exact_bound(ref):
    """lse = log n from an fp32 log: a few fp32 ulps."""
    return 2.0 ** -20 * ref.abs().clamp_min(1.0)


class Checker:
    """Collects element-wise comparisons.  Each check() takes got / ref / bound shaped [B, H, L, ...]; an element fails when
    |got - ref| > bound or got is not finite.  The worst error-to-bound ratio of each bar and where it happened are kept in
    .worst, every failing comparison in .failures (one line each, with the worst (b, h, row) and its ratio)."""

    def __init__(self):
        self.failures = []
        self.worst = {}

    def check(self, bar, got, ref, bound, ctx):
        got = got.to(F64)
        ref, bound = ref.to(got.device), bound.to(got.device)
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, math.inf))
        B, H, L = ratio.shape[:3]
        per_row = ratio.reshape(B, H, L, -1).amax(-1)
        flat = int(per_row.argmax())
        worst = float(per_row.reshape(-1)[flat])
        b, h, row = flat // (H * L), (flat // L) % H, flat % L
        where = f"{ctx} b={b} h={h} row={row}"
        if worst > self.worst.get(bar, (-1.0, ""))[0]:
            self.worst[bar] = (worst, where)
        if not worst <= 1.0:
            self.failures.append(f"{bar}: {where}: error/bound {worst:.3g}")
        return worst

    def ok(self):
        return not self.failures

    def report(self, limit=40):
        lines = [f"{len(self.failures)} failing comparisons"] + self.failures[:limit]
        lines += ["worst error/bound per bar:"] + [f"  {k}: {v[0]:.3g} at {v[1]}" for k, v in sorted(self.worst.items())]
        return "\n".join(lines)
