"""Float64 restatements of the frozen-affine LayerNorm kernels (csrc/layernorm.hip: forward, backward, its three-byte and periodic variants), of the
LayerNorm + row pool of csrc/dino_pool.hip (uia_ln_mean_rows) and of the three-byte codec of csrc/uia_common.h, the bounds that judge the kernels, the
case tables and the conditions on the inputs.  A plain module, no pytest: tests/test_layernorm_contract_gpu.py runs the kernels next to these
functions; tests/test_layernorm_reference_host.py checks every restatement against a second form, proves the codec's error figures over a sweep of bit
patterns, runs an fp32 emulation of the kernels' order of operations against the bounds and shows that planted bugs exceed them.

The restatements take CPU tensors holding exactly what the kernel sees (dy already rounded to the storage type, three-byte operands decoded, eps rounded
to fp32) and return Term(ref, mag) per output.  An element is judged by

    |got − ref| ≤ u·mag + u_out·|ref| (+ A3 for a three-byte result),      u = 2^-24,     bound() below,

first order in u.  u_out: 2^-24 (fp32), 2^-8 (bf16), U3 = 2^-15 (three-byte, with the absolute A3 = 256·2^-149 for subnormal results).  mag holds, in
units of u, every rounding of the kernel on the magnitude it acts on.  No constant here comes from a GPU result; the worst error/bound of the fp32
emulation of the host test stands beside each count.

Derivation (line numbers of csrc/layernorm.hip; the backward :81-162 and the pool dino_pool.hip:30-55 repeat the forward's statistics).
  a1 = mean|x| of the row, r = 1/sqrt(var + eps), x̂ = (x − μ)·r, all in float64.
  mean    a lane adds its ≤ 16 values :33-37 (4 float4, ((v0 + v1) + v2) + v3 onto s), wave_sum adds six butterfly levels (uia_common.h:260-272), / D is one
          correctly rounded division :38.  |δμ| ≤ C_MEAN·u·a1, C_MEAN = 16 + 6 + 1.
  var     d = x − μ̂ (1 rounding, so 2 on d²), 16 fma per lane :45, six levels, / D and + eps :48: every term is positive, so the roundings are a relative
          C_VAR·u = (2 + 16 + 6 + 1 + 1)·u on var + eps.  The error of the mean enters exactly as + δμ² (the cross term Σ(x − μ)·δμ is zero):
          relative ρ = (C_MEAN·u·a1·r)² on var + eps, and only upwards.
  rstd    rsqrtf: one ulp (2u) is what AMD's ISA document states for v_rsq_f32 and the HIP math table for rsqrtf; half the variance's relative error:
          |δr| ≤ r·(C_RSTD·u + ρ/2), C_RSTD = C_VAR/2 + 2 = 15  (1 − 1/sqrt(1 + ρ) ≤ ρ/2 for every ρ ≥ 0, so constant rows with a tiny eps are covered).
  x̂       (x − μ̂)·r̂: the subtraction and the product are one rounding each, r̂ carries its own error, and δμ shifts every element by r·δμ, the
          CONDITIONING term:   xm = C_MEAN·a1·r + |x̂|·(C_XHAT + ρ/2u),  C_XHAT = 1 + C_RSTD + 1 = 17.
          Rows far from zero (a1·r large) and constant rows (x̂ = 0, a1·r = |c|/sqrt(eps)) are judged by this term, not left out.
  y       fma(x̂, γ, β) :57, one rounding on |x̂·γ| + |β|:      mag_y = |γ|·xm + |x̂·γ| + |β|.       stats :49: mag_mean = C_MEAN·a1, mag_rstd = r·(C_RSTD + ρ/2u).
  dx      g = dy·γ (1) :112.  mean(g) :135/:138: ≤ 16 adds, six levels, / D on g's own rounding: (C_MEAN + 1)·u·mean|g|.  mean(g·x̂) :136/:138: the same
          count on mean|g·x̂| plus x̂'s error inside, mean(|g|·xm).  The bracket b = g − mean(g) − x̂·mean(g·x̂) :153 is three operations on |b|_mag =
          |g| + mean|g| + |x̂|·mean|g·x̂|; r̂·b one more with r̂'s own error; the add onto dres one more (contracted into fma by the compiler or not: no more
          roundings than counted).  x̂·mean(g·x̂) by the product rule, one factor's error at a time:
          mag_dx = |dres| + r·( |g| + (C_MEAN + 1)·mean|g| + xm·mean|g·x̂| + |x̂|·((C_MEAN + 1)·mean|g·x̂| + mean(|g|·xm)) + (C_BRACKET + ρ/2u)·|b|_mag ),
          C_BRACKET = 3 + 1 + C_RSTD + 1 = 20.
  pool    x̂ as above; a wave adds its ≤ ceil(per/4) rows of a slice of per = ceil(n/32) rows :54, the four waves are added in order :65-70, the 32 slices in
          order dino_pool.hip:83-86 (depth S = ceil(per/4) + 3 + 32), inv = 1/n and the product (2), the fma onto β (1) :90:
          mag = |γ|/n·Σ_l (xm_l + S·|x̂_l|) + 2·|γ|·|mean x̂| + |γ·mean x̂| + |β|.

Worst error/bound of the fp32 emulation (tests/test_layernorm_reference_host.py, the whole case tables, correctly rounded rsqrt and division):
  forward  y fp32 0.323, y bf16 0.993, mean 0.134, rstd 0.152;      backward  dx fp32 0.483, dx bf16 0.994;
  three-byte  dx32 0.467, decoded (hi, lo) 0.931, hi plane 0.995, dxT 0.995;      periodic  fp32 0.476, three-byte 0.927;      pool 0.378.
(The bf16 figures are the stored value's own rounding meeting u_out = 2^-8 just above a power of two, the three-byte ones a clamped low byte meeting
U3 = 2^-15 in the same way; the fp32 figures say the counts, worst cases of every chain, stay a factor 2 to 7 above what round-to-nearest does here.)

Three-byte codec (uia_common.h:64-98), from the bit arithmetic.  With vb the float's bits and L = vb & 0xFFFF:
  hi = round-to-nearest-even of vb to its top 16 bits (bf16);  d = ((vb + 0x80) >> 8) − (hi << 8) is the 24-bit rounding of vb minus the hi plane:
  d = (L + 0x80) >> 8 ∈ [0, 128] where hi rounded down, d = ((L + 0x80) >> 8) − 256 ∈ [−128, 0] where it rounded up.  lo = clamp(d, −127, 127).
  decode: bits = (hi << 16) + (lo << 8).  Where d was not clamped the decoded bits are vb rounded to a multiple of 256: at most 128 ulp of x away
  (the rounded value never passes the next power of two, a multiple of 2^23): relative ≤ 128·2^-23 = 2^-16.  d = 128 (L in [0x7F80, 0x8000], hi rounded
  down) and d = −128 (L in [0x8000, 0x807F], hi rounded up) are clamped: one step of 256 more, at most 256 ulp: relative ≤ 2^-15, reached but for the
  factor 1/(1 + 2^-8) at L = 0x8000 on an even hi with a zero mantissa (1.992·2^-16).  Subnormal x: the same steps of 2^-149, absolute ≤ 256·2^-149.
  Sign and order: the codec acts on the magnitude bits only (decode∘encode is odd) and is monotone on finite inputs.
  Overflow: the hi plane is the round-to-nearest bf16, so finite |x| with bits ≥ 0x7F7F8000 (3.39618e38) have an INFINITE hi plane (the T copy a GEMM
  reads), and from bits 0x7F7FFF80 (3.40280e38) on the decoded value is inf as well.  Input condition: |x| < 0x7F7F8000 as bits (THREE_MAX).

Input conditions (asserted for every case by the host test): finite rows; Σ(x − μ)² < 2^127; three-byte operands below THREE_MAX.
"""
import math
from collections import namedtuple

import torch

import helpers_reference as R

F64, F32, BF16, I8 = torch.float64, torch.float32, torch.bfloat16, torch.int8
U = 2.0 ** -24
U3 = 2.0 ** -15                     # three-byte result, low byte clamped (2^-16 where it is not)
U3_UNCLAMPED = 2.0 ** -16
A3 = 256 * 2.0 ** -149              # three-byte result in fp32's subnormal range
THREE_MAX_BITS = 0x7F7F8000         # the first magnitude whose hi plane is inf
THREE_INF_BITS = 0x7F7FFF80         # the first magnitude that decodes to inf
THREE = "three"
POOL_SLICES = 32

C_MEAN = 16 + 6 + 1
C_VAR = 2 + 16 + 6 + 1 + 1
C_RSTD = C_VAR // 2 + 2
C_XHAT = 1 + C_RSTD + 1
C_BRACKET = 3 + 1 + C_RSTD + 1

Term = namedtuple("Term", "ref mag")


def bound(term, out=F32):
    """u·mag + u_out·|ref|; out: torch.float32, torch.bfloat16 or THREE (the decoded three-byte result)."""
    if out == THREE:
        return U * term.mag + U3 * term.ref.abs() + A3
    return R.bound(term.ref, term.mag, 1, out)


def eps32(eps):
    """eps as the kernel receives it (a float argument)."""
    return float(torch.tensor(eps, dtype=F32))


def nv_bwd(D):
    """uia_layernorm_bwd3_launch / _periodic_launch: float4 per lane of the instantiation."""
    return 3 if D <= 768 else 4


NV_FWD = 4                          # LN_MAXV, POOL_V


# ------------------------------------------------------------------------------------------ LayerNorm
def _stats(x, eps):
    x = x.to(F64)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    r = 1 / torch.sqrt(var + eps32(eps))
    xhat = (x - mu) * r
    a1 = x.abs().mean(-1, keepdim=True)
    rho_u = (C_MEAN * a1 * r) ** 2 * U / 2                       # ρ/2 in units of u
    xm = C_MEAN * a1 * r + xhat.abs() * (C_XHAT + rho_u)
    return mu, r, xhat, a1, rho_u, xm


def ln_fwd(x, gamma, beta, eps):
    """y = x̂·γ + β, mean and rstd of uia_layernorm_fwd_stats on x [M, D]: dict y / mean / rstd -> Term."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    mu, r, xhat, a1, rho_u, xm = _stats(x, eps)
    y = xhat * gamma + beta
    return dict(y=Term(y, gamma.abs() * xm + (xhat * gamma).abs() + beta.abs()),
                mean=Term(mu[..., 0], C_MEAN * a1[..., 0]), rstd=Term(r[..., 0], (r * (C_RSTD + rho_u))[..., 0]))


def ln_bwd(dy, x, gamma, eps, dres=None):
    """dx = dres + rstd·(g − mean(g) − x̂·mean(g·x̂)), g = dy·γ  (the header of csrc/layernorm.hip): Term."""
    gamma = gamma.to(F64)
    mu, r, xhat, a1, rho_u, xm = _stats(x, eps)
    g = dy.to(F64) * gamma
    m = lambda v: v.mean(-1, keepdim=True)                                                                             # noqa: E731
    ref = r * (g - m(g) - xhat * m(g * xhat))
    mgx = m((g * xhat).abs())
    bmag = g.abs() + m(g.abs()) + xhat.abs() * mgx
    mag = r * (g.abs() + (C_MEAN + 1) * m(g.abs()) + xm * mgx + xhat.abs() * ((C_MEAN + 1) * mgx + m(g.abs() * xm)) + (C_BRACKET + rho_u) * bmag)
    if dres is not None:
        ref, mag = ref + dres.to(F64), mag + dres.to(F64).abs()
    return Term(ref, mag)


def ln_bwd_periodic(dy, x, gamma, eps, dres_rows, period):
    """ln_bwd whose residual gradient exists on the rows r % period == 0 only: dres_rows [ceil(M / period), D] compact."""
    t = ln_bwd(dy, x, gamma, eps)
    ref, mag = t.ref.clone(), t.mag.clone()
    M = ref.shape[0]
    assert dres_rows.shape[0] == -(-M // period)
    ref[0::period] += dres_rows.to(F64)
    mag[0::period] += dres_rows.to(F64).abs()
    return Term(ref, mag)


def pool_depth(n):
    per = -(-n // POOL_SLICES)
    return -(-per // 4) + 3 + POOL_SLICES


def ln_mean_rows(x, gamma, beta, eps, row0, n):
    """out[b] = mean over rows row0 .. row0 + n − 1 of LayerNorm(x[b, l]) on x [B, L, D] (uia_ln_mean_rows): Term [B, D]."""
    gamma, beta = gamma.to(F64), beta.to(F64)
    mu, r, xhat, a1, rho_u, xm = _stats(x[:, row0:row0 + n], eps)
    mean = xhat.mean(1)
    mag = gamma.abs() * (xm + pool_depth(n) * xhat.abs()).mean(1) + 2 * (gamma * mean).abs() + (gamma * mean).abs() + beta.abs()
    return Term(mean * gamma + beta, mag)


# ------------------------------------------------------------------------------------------ the three-byte codec
def bits_of(x):
    """fp32 -> its bits as non-negative int64."""
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def float_of(bits):
    """int64 bits (taken mod 2^32) -> fp32."""
    b = bits & 0xFFFFFFFF
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(F32)


def _bf16_of(hs):
    hs = hs & 0xFFFF
    return torch.where(hs >= 2 ** 15, hs - 2 ** 16, hs).to(torch.int16).view(BF16)


def hi_bits(hi):
    return hi.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def encode3(x, bug=None):
    """three_byte_store4: (hi bf16, lo int8) of fp32 x (not NaN).  bug: "hi_truncated", "no_clamp" (planted, for the host test)."""
    vb = bits_of(x)
    hs = (vb >> 16) if bug == "hi_truncated" else ((vb + 0x7FFF + ((vb >> 16) & 1)) >> 16)
    d = ((vb + 0x80) >> 8) - (hs << 8)
    d = ((d + 128) % 256) - 128 if bug == "no_clamp" else d.clamp(-127, 127)
    return _bf16_of(hs), d.to(I8)


def decode3(hi, lo, bug=None):
    """three_byte_load4 / three_byte_decode4 / rows3_kernel: float bits = (hi bits << 16) + (sign-extended lo << 8).  bug: "zero_extended"."""
    lo = lo.to(torch.int64)
    if bug == "zero_extended":
        lo = lo & 0xFF
    return float_of((hi_bits(hi) << 16) + (lo << 8))


KB = 32                             # bf16 elements of a 64-byte column block


def kblock(hi, rows_total, fill=float("nan")):
    """The K-blocked hi plane [D/32, rows_total, 32] of a row-major [M, D] plane; rows M .. rows_total hold `fill`."""
    M, D = hi.shape
    assert D % KB == 0 and rows_total >= M
    out = torch.full((D // KB, rows_total, KB), fill, dtype=hi.dtype)
    out[:, :M] = hi.reshape(M, D // KB, KB).permute(1, 0, 2)
    return out


def unkblock(kb, M, rows_in_address=None):
    """The row-major [M, D] plane of a K-blocked one, element (row, c) read at ((c >> 5)·kb_rows + row)·32 + (c & 31) of the flat plane, as the kernels
    address it.  rows_in_address: the row count used in the address (a planted bug uses M)."""
    nb, rows_total, g = kb.shape
    kr = rows_total if rows_in_address is None else rows_in_address
    flat = kb.reshape(-1)
    c = torch.arange(nb * g)
    idx = ((c >> 5)[None, :] * kr + torch.arange(M)[:, None]) * KB + (c & 31)[None, :]
    return flat[idx]


# ------------------------------------------------------------------------------------------ operands
KINDS = ("normal", "far", "const", "zero", "outlier", "small")


def rnd(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).float()


def rows(M, D, seed, first=0):
    """fp32 [M, D]: row i is of kind KINDS[(i + first) % 6]: N(0.5, 2); 1000 + N(0, 1); a constant; zero; N(0, 1) with one 1e4 outlier; 1e-3·N(0, 1)."""
    z = rnd(M, D, seed=seed)
    out = torch.zeros(M, D)
    for i in range(M):
        k = KINDS[(i + first) % 6]
        if k == "normal":
            out[i] = 0.5 + 2 * z[i]
        elif k == "far":
            out[i] = 1000 + z[i]
        elif k == "const":
            out[i] = 0.7 * (1 + i % 3)
        elif k == "outlier":
            out[i] = z[i]
            out[i, (7 * i + seed) % D] = 1e4
        elif k == "small":
            out[i] = 1e-3 * z[i]
    return out.float()


def affine(D, seed):
    """γ ~ N(1, 0.3), β ~ N(0, 0.3) with zeros and negative values planted."""
    gamma, beta = rnd(D, seed=seed + 1, scale=0.3, shift=1.0), rnd(D, seed=seed + 2, scale=0.3)
    gamma[0], gamma[1], gamma[D - 1] = 0.0, -1.5, -0.5
    beta[0], beta[2] = 0.0, -1.0
    return gamma, beta


def ld_of(kind, D):
    return {"D": D, "D+4": D + 4, "7D": 7 * D}[kind]


def check_conditions(x):
    """The input conditions of the module docstring on fp32 rows."""
    assert bool(torch.isfinite(x).all())
    x = x.to(F64)
    assert float(((x - x.mean(-1, keepdim=True)) ** 2).sum(-1).max()) < 2.0 ** 127


def check_three(x):
    assert int((bits_of(x) & 0x7FFFFFFF).max()) < THREE_MAX_BITS


WIDTHS = (4, 64, 252, 256, 260, 768, 772, 1024)
ROWS = (1, 3, 4, 5, 37)
EPSS = (1e-5, 1e-6, 1e-12)
DTYPES = (F32, BF16)
FWD_OUTS = (("yT",), ("y32",), ("yT", "y32"), ("stats",), ("yT", "y32", "stats"))
FWD_LD = ("D", "D+4", "7D")
BWD_OUTS = (("dx32",), ("dxT",), ("dx32", "dxT"))
BWD_LD = ("D", "D+4")

FwdCase = namedtuple("FwdCase", "dtype M D ld eps outs first")
BwdCase = namedtuple("BwdCase", "dtype M D ld eps dres outs first")
ThreeCase = namedtuple("ThreeCase", "M D eps x dres outs kb_extra first")
PeriodicCase = namedtuple("PeriodicCase", "form M period D eps kb_extra first")
PoolCase = namedtuple("PoolCase", "B n row0 L D eps first")


def fwd_cases():
    return [FwdCase(dt, ROWS[(i + j + 2 * p) % 5], D, FWD_LD[(i + j + p) % 3], EPSS[(i + 2 * j + p) % 3], FWD_OUTS[(i + 2 * j + 3 * p) % 5], i + p)
            for p in range(2) for j, dt in enumerate(DTYPES) for i, D in enumerate(WIDTHS)]


def bwd_cases():
    return [BwdCase(dt, ROWS[(i + 2 * j + 3 * p) % 5], D, BWD_LD[(i + j + p) % 2], EPSS[(i + j + 2 * p) % 3], bool((i // 2 + p) % 2), BWD_OUTS[(i + j + p) % 3], i + 2 * p)
            for p in range(2) for j, dt in enumerate(DTYPES) for i, D in enumerate(WIDTHS)]


THREE_D = (4, 260, 768, 772, 1024)
THREE_D_KB = (32, 768, 1024)
THREE_OUTS = (("dx32", "dxT"), ("dxT", "dx_lo"), ("dx32", "dxT", "dx_lo"))


def _three_forms(kb):
    out = []
    for x in ("f32", "rm", "kb"):
        for dres in ("none", "f32", "rm", "kb"):
            for outs in THREE_OUTS:
                three = x != "f32" or dres in ("rm", "kb") or "dx_lo" in outs
                if three and (("kb" in (x, dres)) == kb):
                    out.append((x, dres, outs))
    return out


def three_cases():
    out = [ThreeCase(ROWS[(n + n // 5) % 5], THREE_D[n % 5], EPSS[n % 3], x, dres, outs, 0, n) for n, (x, dres, outs) in enumerate(_three_forms(False))]
    out += [ThreeCase(ROWS[(n + n // 3) % 5], THREE_D_KB[n % 3], EPSS[(n + 1) % 3], x, dres, outs, (0, 3)[n % 2], n) for n, (x, dres, outs) in enumerate(_three_forms(True))]
    return out


PERIODIC_M = (1, 5, 11)
PERIODIC_FORMS = ("f32", "bf16", "bf16x3")            # fp32; bf16 with fp32 x; bf16 with three-byte x (K-blocked where D % 32 == 0)


def periods_of(M):
    return sorted({1, 2, 5, M, M + 1})


def periodic_cases():
    out, n = [], 0
    for M in PERIODIC_M:
        for period in periods_of(M):
            for form in PERIODIC_FORMS:
                out.append(PeriodicCase(form, M, period, THREE_D[n % 5], EPSS[n % 3], 2 * (n % 2), n))
                n += 1
    return out


POOL_N = (1, 2, 31, 32, 33, 63, 65, 257)
POOL_D = (4, 260, 1024)
POOL_B = (1, 3)


def pool_cases():
    out = []
    for i, n in enumerate(POOL_N):
        L = n + 2
        for k, row0 in enumerate((0, 1, L - n)):
            out.append(PoolCase(POOL_B[(i + k) % 2], n, row0, L, POOL_D[(i + k) % 3], EPSS[(i + 2 * k) % 3], i + k))
    return out


def name_of(case):
    dt = lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else v                                    # noqa: E731
    return type(case).__name__ + "(" + ", ".join(f"{k}={dt(v)}" for k, v in case._asdict().items()) + ")"


def seed_of(case):
    return 17 * case.D + 1000 * getattr(case, "M", getattr(case, "n", 0)) + case.first


def fwd_inputs(case):
    """x [M, D] fp32, γ, β."""
    s = seed_of(case)
    return (rows(case.M, case.D, s, case.first),) + affine(case.D, s)


def bwd_inputs(case, dtype=None):
    """dy (rounded to the launch dtype, upcast), x, γ, dres or None."""
    s = seed_of(case)
    dt = dtype or case.dtype
    dy = rnd(case.M, case.D, seed=s + 3).to(dt).float()
    dres = rnd(case.M, case.D, seed=s + 4) if case.dres not in (False, "none") else None
    return dy, rows(case.M, case.D, s, case.first), affine(case.D, s)[0], dres


def three_inputs(case):
    """dy (bf16 values), x as the kernel sees it, γ, dres as the kernel sees it (or None), and the planes: dict x_hi / x_lo / dres_hi / dres_lo (row-major)."""
    dy, x, gamma, dres = bwd_inputs(case, BF16)
    planes = {}
    if case.x != "f32":
        planes["x_hi"], planes["x_lo"] = encode3(x)
        x = decode3(planes["x_hi"], planes["x_lo"])
    if case.dres in ("rm", "kb"):
        planes["dres_hi"], planes["dres_lo"] = encode3(dres)
        dres = decode3(planes["dres_hi"], planes["dres_lo"])
    return dy, x, gamma, dres, planes


def periodic_inputs(case):
    """dy, x as the kernel sees it, γ, dres_rows [ceil(M / period), D], planes (x_hi / x_lo for the three-byte form)."""
    s = seed_of(case)
    dt = F32 if case.form == "f32" else BF16
    dy = rnd(case.M, case.D, seed=s + 3).to(dt).float()
    x, gamma = rows(case.M, case.D, s, case.first), affine(case.D, s)[0]
    dres_rows = rnd(-(-case.M // case.period), case.D, seed=s + 5)
    planes = {}
    if case.form == "bf16x3":
        planes["x_hi"], planes["x_lo"] = encode3(x)
        x = decode3(planes["x_hi"], planes["x_lo"])
    return dy, x, gamma, dres_rows, planes


def pool_inputs(case):
    """x [B, L, D], γ, β."""
    s = seed_of(case)
    return (rows(case.B * case.L, case.D, s, case.first).reshape(case.B, case.L, case.D),) + affine(case.D, s)


# ------------------------------------------------------------------------------------------ the codec's bit patterns
LOW_HALVES = (0x0000, 0x0001, 0x007F, 0x0080, 0x0081, 0x00FF, 0x0100, 0x7F7F, 0x7F80, 0x7F81, 0x7FFF, 0x8000, 0x8001, 0x807F, 0x8080, 0x8081, 0xFF7F, 0xFF80, 0xFFFF)
LOW_BYTES = (-128, -127, -126, -65, -64, -63, -2, -1, 0, 1, 2, 63, 64, 65, 126, 127, -100, 100, 37)
assert len(LOW_HALVES) == len(LOW_BYTES) == 19


def sweep_bits():
    """All 65 536 upper halves × the 19 lower halves around every edge of the encoder: int64 [65536·19]."""
    return ((torch.arange(65536, dtype=torch.int64) << 16)[:, None] + torch.tensor(LOW_HALVES, dtype=torch.int64)[None, :]).reshape(-1)


def sweep_values(limit_bits=THREE_MAX_BITS):
    """The sweep's fp32 values a three-byte tensor may hold: finite, magnitude bits below limit_bits, no −0.0."""
    b = sweep_bits()
    mag = b & 0x7FFFFFFF
    return float_of(b[(mag < limit_bits) & (b != 0x80000000)])


def sweep_planes():
    """(hi, lo) for every hi pattern × the 19 low bytes whose decoded value is finite and not −0.0."""
    hs = torch.arange(65536, dtype=torch.int64)[:, None].expand(65536, 19).reshape(-1)
    lo = torch.tensor(LOW_BYTES, dtype=torch.int64)[None, :].expand(65536, 19).reshape(-1)
    bits = ((hs << 16) + (lo << 8)) & 0xFFFFFFFF
    keep = ((bits & 0x7F800000) != 0x7F800000) & (bits != 0x80000000)
    return _bf16_of(hs[keep]), lo[keep].to(I8)


def pad_rows(v, D, fill):
    """A flat tensor as [ceil(len / D), D], the tail filled."""
    n = -(-v.numel() // D) * D
    out = torch.full((n,), fill, dtype=v.dtype)
    out[:v.numel()] = v
    return out.reshape(-1, D)


assert math.isclose(float(float_of(torch.tensor([THREE_MAX_BITS]))[0]), 3.39617752923046e38)
