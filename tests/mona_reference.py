"""Float64 restatements of the Mona spatial operator and the plain pre-norm (csrc/mona.hip, csrc/mona_spatial.h), forward and backward,
the bounds that judge the kernels, the case tables and the launcher's own decision formulas.  A plain module, no pytest:
tests/test_mona_contract_gpu.py runs the kernels next to these functions, tests/test_mona_reference_host.py checks every restatement against
float64 autograd through oracle/mona_ref.py and shows on the CPU that the bounds catch planted bugs.

The restatements are explicit (no autograd).  They take CPU tensors holding exactly the operands the kernel sees: t, dd and du already rounded
to the storage type and upcast, parameters in fp32 upcast.  Every function returns a dict  name -> Term(ref, mag, a, mf):

    ref   the float64 value
    mag   the sum of the absolute values of the terms that make up the element, stage by stage: each linear stage is evaluated again on absolute
          values, with the softmax mixing weights, rstd and x̂ held at their reference values; through GELU with the global Lipschitz constants
          GP1 = max|gelu'| and GP2 = max|gelu''| below.  The pre-norm terms hold Σ|terms| and take one count C per output (C_U, C_DX, c_pre_sum).
          The spatial terms hold Σ over the stages of (the stage's count of fp32 roundings)·Σ|terms of that stage|, carried through the later
          stages' absolute values (class Err): C·mag with every stage's count on its own magnitude.  A single C on the last stage's nested
          magnitude is the same sum with the largest count on everything, and at 14 × 14 it reached the size of the gradients themselves.
    a     the absolute term: the GELU approximation error (A_PHI, A_DPHI below), carried through the later linear stages on absolute values
    mf    Σ|a||b| of the bf16 matrix-core products the element depends on (the projector, its data gradient, its weight gradient), carried
          through the later stages in the same way.  Used only where the launcher takes the fast kernel (fast_path below).

An element is judged by   |got − ref| ≤ C·u·mag + a + u_mfma·mf + u_out·|ref|   (bound()), first order in u.  No constant here comes from a GPU result.

Operand scales: those of tests/test_lora_contract_gpu.py::test_mona_seeded_launches_equal_the_host_mask, except projector.weight at 0.125
instead of 0.2: with 0.2 the standard deviation of z is about 2 and |z| ≤ 8 (asserted by the host test) fails at 14 × 14.
"""
import math
from collections import namedtuple

import torch

F64 = torch.float64
F32 = torch.float32
BF16 = torch.bfloat16
U = 2.0 ** -24
# Both operands of a matrix-core product rounded to bf16, at 2^-9 each: (1 + 2^-9)² − 1, on Σ|a||b|.  Round-to-nearest to bf16's 8 significant bits can be
# off by up to 2^-8 of one value (U_OUT[bf16] of helpers_reference), so a sum of very few products can pass this figure: the projector's weight gradient
# did, by 18 %, at 1 x 4 with two images, and has since been formed from hi + lo operand pairs (3·2^-16, mona.hip's dP phase).  The projector and its data
# gradient are sums of 64 products of operands rounded once and stay below it at every case of the tables.  The weight gradient's own term (own_mf in
# spatial_bwd) is kept at this figure: more than the hi + lo form needs, no more than the suite was asked to allow.
U_MFMA = 2 * 2.0 ** -9 + 2.0 ** -18
BOTT = 64
VARIANTS = ("baseline", "noise_aware", "freq_enhanced", "hybrid")
KEYS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "proj_w", "proj_b", "freq", "ne1_w", "ne1_b", "ne3_w", "ne3_b")
ORACLE_NAMES = dict(conv1_w="adapter_conv.conv1.weight", conv1_b="adapter_conv.conv1.bias", conv2_w="adapter_conv.conv2.weight",
                    conv2_b="adapter_conv.conv2.bias", conv3_w="adapter_conv.conv3.weight", conv3_b="adapter_conv.conv3.bias",
                    proj_w="adapter_conv.projector.weight", proj_b="adapter_conv.projector.bias", freq="adapter_conv.freq_filter",
                    ne1_w="adapter_conv.noise_estimator.1.weight", ne1_b="adapter_conv.noise_estimator.1.bias",
                    ne3_w="adapter_conv.noise_estimator.3.weight", ne3_b="adapter_conv.noise_estimator.3.bias")
ORACLE_SHAPES = dict(conv1_w=(64, 1, 3, 3), conv2_w=(64, 1, 5, 5), conv3_w=(64, 1, 7, 7), proj_w=(64, 64, 1, 1), ne1_w=(16, 64, 1, 1), ne3_w=(3, 16, 1, 1))

Term = namedtuple("Term", "ref mag a mf")


def has_freq(variant):
    return variant in ("freq_enhanced", "hybrid")


def has_noise(variant):
    return variant in ("noise_aware", "hybrid")


def keys_of(variant):
    return KEYS[:8] + (("freq",) if has_freq(variant) else ()) + (KEYS[9:] if has_noise(variant) else ())


# ------------------------------------------------------------------------------------------ GELU: constants and their derivation
# gelu(x) = x·Φ(x), gelu'(x) = Φ(x) + x·φ(x), gelu''(x) = φ(x)·(2 − x²), gelu'''(x) = φ(x)·x·(x² − 4), with φ the normal density.
#   max|gelu'|:  gelu'' = 0 at x = ±√2;  gelu'(√2) = Φ(√2) + √2·φ(√2) = 0.921350 + 0.207554 = 1.128904  (gelu'(−√2) = −0.1289, and → 0 / 1 outside)
#   max|gelu''|: gelu''' = 0 at x = 0, ±2;  gelu''(0) = 2·φ(0) = 2/√(2π) = 0.797885,  |gelu''(±2)| = 2·φ(2) = 0.107982
# Both are global Lipschitz constants (of gelu and of gelu'), so an input error δ of any size moves the result by at most GP·|δ|: no remainder term.
GP1 = 1.128905
GP2 = 0.797885
# gelu_parts<false> (csrc/uia_common.h:163-179):  ax = |x|·0.70710678f;  E = __expf(−ax·ax) = v_exp(−ax²·log2e);  t = v_rcp(fma(0.3275911, ax, 1));
# y = Horner(t) (4 fma) · t;  half = 0.5·y·E;  Φ = 1 − half or half.  Errors of Φ, in units of u = 2^-24 unless stated:
#   Abramowitz–Stegun 7.1.26: |Δerf| ≤ 1.5e-7 in exact arithmetic, so |ΔΦ| ≤ 0.75e-7                                                    A_AS
#   ax: the product and the constant, 2u relative.  ax²: 5u relative; · log2e (product, constant): 7u relative on the exponent a = ax²·log2e, an
#     absolute 7u·a there, i.e. 7u·ax² relative on E = 2^-a.  s·e^-s ≤ 1/e for s = ax² ≥ 0:  |δE| ≤ 7u/e + (v_exp's rounding, u·E ≤ u) = 3.6u
#   t: the fma u, its argument error 0.3275911·ax·2u/(1 + 0.3275911·ax) ≤ 2u, v_rcp's rounding u: 4u relative, t ≤ 1.  |dy/dt| ≤ DY on [0, 1]
#     (evaluated below from the polynomial): DY·4u.  Horner: 4 fma and the product, each u·|intermediate| ≤ 1.4532u, later factors t ≤ 1: 7.3u
#   half = 0.5·y·E, y ≤ 1, E ≤ 1: 0.5·(δy + δE) + 0.5u for the product;  Φ = 1 − half: u.
#   hardware terms: one further ulp (2u relative) each for v_exp_f32 and v_rcp_f32 beyond a correctly rounded result.  This project's documents hold no
#     accuracy figure for either; one ulp is what AMD's ISA documents state for both, and is what is assumed here:
#     v_exp: 0.5·y·2u·E ≤ u;  v_rcp: 0.5·DY·2u·t ≤ DY·u.
_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
_tt = torch.linspace(0, 1, 100001, dtype=F64)
DY = float(sum((k + 1) * a * _tt ** k for k, a in enumerate(_AS)).abs().max())         # 3.44 at t = 1
A_AS = 0.75e-7
A_PHI_ROUND = (0.5 * (DY * 4 + 7.3 + 3.6) + 0.5 + 1) * U
A_PHI_HW = (1 + DY) * U
A_PHI = A_AS + A_PHI_ROUND + A_PHI_HW
# gelu' = fma(x·0.39894228f, E, Φ):  ΔΦ;  |x|·0.3989·|δE| with |δE| ≤ 7u·ax²·E + u·E:  √(2s)·s·e^-s ≤ 0.5797 (s = 1.5) and |x|·e^(-x²/2) ≤ e^-½ = 0.6065:
# 0.3989·(7·0.5797 + 0.6065)u = 1.87u;  x·0.3989 (product, constant) 2u relative: 0.3989·0.6065·2u = 0.49u;  the fma, |gelu'| ≤ GP1: 1.13u.
# Hardware: v_exp's further ulp 0.3989·0.6065·2u = 0.49u.
A_DPHI_ROUND = A_PHI_ROUND + (1.87 + 0.49 + 1.13) * U
A_DPHI_HW = A_PHI_HW + 0.49 * U
A_DPHI = A_AS + A_DPHI_ROUND + A_DPHI_HW


def gelu(z):
    return z * 0.5 * (1 + torch.erf(z / math.sqrt(2)))


def dgelu(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def gelu_parts_f32(x):
    """gelu_parts<false> operation by operation in torch fp32 on the CPU, with a correctly rounded exp2 and reciprocal: (x·Φ, gelu')."""
    x = x.to(F32)
    f = lambda v: torch.tensor(v, dtype=F32)                                                                          # noqa: E731
    fma = lambda a, b, c: (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)         # one rounding (a·b is exact in float64; the double rounding of the sum is below 2^-29 relative)  # noqa: E731
    ax = x.abs() * f(0.70710678118654752)
    arg = (-ax * ax) * f(1.4426950408889634)
    E = torch.exp2(arg.to(F64)).to(F32)
    t = (1.0 / fma(f(0.3275911), ax, f(1.0)).to(F64)).to(F32)
    y = fma(f(1.061405429), t, f(-1.453152027))
    y = fma(y, t, f(1.421413741))
    y = fma(y, t, f(-0.284496736))
    y = fma(y, t, f(0.254829592)) * t
    half = f(0.5) * y * E
    Phi = torch.where(x >= 0, 1.0 - half, half)
    return x * Phi, fma(x * f(0.39894228040143268), E, Phi)


# ------------------------------------------------------------------------------------------ the launcher's decisions (mona.hip, mona_spatial.h)
LDS_LIMIT = 160 * 1024
NGRP = 8
SCR_SIZE = 720
RED_FLOATS = 64 * 50
FLD = 68
FAST_RED = 4 * 64 * 51
KW_FLOATS = 64 * (9 + 25 + 49)
PRE_GRID_CAP = 1024
REFUSAL = "{h}x{w} grid does not fit the 160 KiB LDS tile"


def spatial_lds(hw, bwd):
    """mona.hip spatial_lds: bytes of the per-pixel kernel's tile."""
    tile = (hw + 1) * BOTT
    cs = max(tile, RED_FLOATS) if bwd else tile
    return (tile * (2 if bwd else 1) + cs + SCR_SIZE) * 4


def spatial_fast_lds(hw, bwd):
    """mona_spatial.h spatial_fast_lds."""
    return ((hw + 1) * BOTT + max(hw * FLD, FAST_RED) + (max((hw + 1) * FLD, KW_FLOATS) if bwd else KW_FLOATS) + SCR_SIZE) * 4


def accepted(h, w, bwd):
    """check_spatial: the per-pixel tile must fit whichever kernel runs."""
    return spatial_lds(h * w, bwd) <= LDS_LIMIT


def fast_path(dtype, h, w, bwd):
    """launch_spatial: bf16, w in {14, 4}, and the fast tile fits (UIA_MONA_FAST unset)."""
    return dtype == BF16 and w in (14, 4) and spatial_fast_lds(h * w, bwd) <= LDS_LIMIT


def largest_h(w, bwd, fast):
    h = 1
    while (fast_path(BF16, h + 1, w, bwd) if fast else accepted(h + 1, w, bwd)):
        h += 1
    return h


def pre_nv(D):
    """uia_mona_pre_bwd_launch: float4 per lane of the instantiation."""
    return 1 if D <= 256 else (3 if D <= 768 else 4)


def pre_accepted(M, D):
    return M > 0 and D > 0 and D % 4 == 0 and D <= 1024


def pre_grid_cap(M):
    """mona_pre_bwd_blocks: the persistent grid before the occupancy cut."""
    return min((M + 3) // 4, PRE_GRID_CAP)


# ------------------------------------------------------------------------------------------ counts of fp32 roundings (C of the bound)
# Counted per stage on its longest dependency chain, from mona.hip / mona_spatial.h (line numbers of the per-pixel kernel; the fast kernel runs the
# same stages in another order and no longer, see each note).  A stage's own roundings are (its count)·u·Σ|terms of the stage|; the errors its
# inputs already carry pass through the stage's absolute values (class Err).  Summed along a chain this is C·u·mag with C the chain's count,
# except that every stage's count multiplies that stage's own magnitude and not the magnitude of everything before it.  Where a chain's length
# depends on how pixels or images are dealt to waves, the count is the number of summands: an upper bound of every order the kernels use.
def n_pool(hw):
    """noise_forward (mona_spatial.h:35-68): a group's <= ceil(hw/8) adds :39, 8 partials :45, f·a and /hw :46."""
    return -(-hw // NGRP) + 8 + 2


N_NE1 = 64          # 64 fma onto the bias, mona_spatial.h:51
N_NE3 = 16          # 16 fma onto the bias :60
N_SOFTMAX = 8       # l − m :64 (1), expf (taken at one ulp: 2), the sum of three (2), the reciprocal (1), the product (2 with the reciprocal's share): a weight's relative error beside 2·|δl|
N_THIRD = 1         # the variants without the estimator: 1.f / 3.f, one rounding
N_CONV = 5 + 49 + 1  # the merged tap KM (3 products, 2 adds: mona_spatial.h:13), 49 fma mona.hip:432, fma(f, acc, bm) :435
N_IDENT = 1         # + t :435
N_PROJ = 64 + 2     # 64 fma on pb :503, + c :505.  (Fast kernel: two MFMAs of 32 products each, + c, + pb.)
N_GELU = 3          # x·Φ or the fma of gelu', 1/(1 − p) :482, · ks :508 / :511
N_DC = 64 + 1       # dc = dz + Pᵀ·dz: 64 fma :556 and the add :558
N_DK_SCALE = 2      # f·red :606, w_k· :612
N_DWM = 49 + 14     # Σ dc·conv_k beyond its hw summands (:590-592): in the fast kernel 49 fma over the taps of dK :949-955; six butterfly levels :624, 8 partials :632
N_DL = 5 + 2        # dot (3 products, 2 adds) :634 and dl = w·(dwv − dot) :635
N_DH = 3            # :640
N_DPOOL = 16 + 1    # :650-651
N_DXF = 5 + 49      # KM and 49 fma :672
N_DT = 1            # fma(f, dxf, dc) :677


def n_img(B):
    """The image sum: <= B adds in mona_ws_reduce_kernel :1092-1102 and the atomic add onto the buffer :1119 (without a workspace: B atomic adds)."""
    return B + 1


# pre-norm (mona.hip:36-76 forward, :220-283 and :389-410 backward)
C_MEAN = 16 + 6 + 1                 # a lane's ≤ 16 adds :49, six butterfly levels of wave_sum, /D :51
C_VAR = 16 + 6 + 1 + 1              # 16 fma :58, six butterfly levels, /D and + eps :61
C_XHAT = C_MEAN + 1 + C_VAR // 2 + 2 + 1                 # x − mean :58; rstd: half the variance's relative error and rsqrtf (taken at one ulp: 2) :61; the product :70
C_U = C_XHAT + 2 + 2                # fma(x̂, w, b) :70; x·γx and the fma :71
# dx: x̂ twice (x̂·mean(g·x̂)); the row sums :250-255; rstd's own relative error on the bracket; γ·w :188 and d·(γw) :249; x̂·mgx, two subtractions, rstd·, the fma, + dy :271
C_DX = 2 * C_XHAT + C_MEAN + (C_VAR // 2 + 2) + 2 + 6


def c_pre_sum(M):
    """A column sum: M summands through a wave's fma chain :245-247, the block's two adds :370/:382, the reduce kernel's eight accumulators and
    their tree :402-405, 16 atomic adds :407-409 onto the buffer; x̂ inside S1; the parameter factor :407-408, and dγ's two sums."""
    return M + 2 + 3 + 16 + C_XHAT + 1 + 1


# ------------------------------------------------------------------------------------------ operands and case tables
def rnd(*shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def spatial_params(variant, kind="A", seed=0):
    """fp32 parameters of one variant.  kind "A": every parameter random; "Z": projector.weight = projector.bias = 0, so that z = c and the
    stencil is judged at fp32 tightness on the fast path too.  The noise estimator's first bias is ±[0.5, 0.7] with alternating signs and its
    first weight small, so that every hidden pre-activation stays away from 0 on both sides of it."""
    s = 100 * seed
    P = dict(conv1_w=rnd(64, 9, seed=s + 1, scale=0.2), conv1_b=rnd(64, seed=s + 2, scale=0.1), conv2_w=rnd(64, 25, seed=s + 3, scale=0.1),
             conv2_b=rnd(64, seed=s + 4, scale=0.1), conv3_w=rnd(64, 49, seed=s + 5, scale=0.05), conv3_b=rnd(64, seed=s + 6, scale=0.1),
             proj_w=rnd(64, 64, seed=s + 7, scale=0.125), proj_b=rnd(64, seed=s + 8, scale=0.1))
    if kind == "Z":
        P["proj_w"], P["proj_b"] = torch.zeros(64, 64), torch.zeros(64)
    if has_freq(variant):
        P["freq"] = rnd(64, seed=s + 9, scale=0.3, shift=1.0)
    if has_noise(variant):
        sign = torch.tensor([1.0, -1.0]).repeat(8)
        P["ne1_w"] = rnd(16, 64, seed=s + 10, scale=0.01)
        P["ne1_b"] = sign * (0.5 + 0.2 * torch.rand(16, generator=torch.Generator().manual_seed(s + 11)))
        P["ne3_w"] = rnd(3, 16, seed=s + 12, scale=0.3)
        P["ne3_b"] = rnd(3, seed=s + 13, scale=0.1)
    return {k: v.float().contiguous() for k, v in P.items()}


DROP_SEEDS = (0x5EED0001, 0x5EED0002)
DROPS = ((0.0, None), (0.1, DROP_SEEDS[0]), (0.5, DROP_SEEDS[1]))


def keep_mask(B, ntok, p, seed):
    if p == 0.0:
        return None
    import lora_reference as LR
    return LR.mona_keep_mask(seed, (B, ntok, BOTT), p)


def spatial_operands(B, h, w, dtype, seed):
    """t, dd ~ N(0, 1) rounded to the storage type."""
    ntok = 1 + h * w
    return rnd(B, ntok, BOTT, seed=1000 + seed).to(dtype), rnd(B, ntok, BOTT, seed=2000 + seed).to(dtype)


# grids (h, w).  Per-pixel kernel, any dtype: fewer pixels than pixel groups; 3×7; (hw + 1)·64 below / at / above RED_FLOATS; a partial last group; hw = 208
PIXEL_GRIDS = ((1, 1), (1, 3), (3, 1), (2, 3), (3, 7), (6, 8), (7, 7), (5, 10), (9, 9), (13, 16))
PIXEL_GRIDS_FP32 = ((5, 4), (14, 14))          # fp32 alone: these widths take the fast kernel in bf16
FAST_H_W4 = (1, 3, 5, 8, 9, 19, 20, 48, 49, 50)
FAST_H_W14 = (1, 5, 6, 9, 14)
IMAGE_SUM_B = (1, 16, 17, 48, 49, 64, 65, 113)
assert (6 * 8 + 1) * 64 < RED_FLOATS == (7 * 7 + 1) * 64 < (5 * 10 + 1) * 64
assert all(fast_path(BF16, h, 4, True) for h in FAST_H_W4) and all(fast_path(BF16, h, 14, True) for h in FAST_H_W14)
assert not any(fast_path(BF16, h, w, False) for h, w in PIXEL_GRIDS)
assert 48 * 4 * FLD <= FAST_RED < 49 * 4 * FLD and 9 * 14 * FLD <= FAST_RED < 14 * 14 * FLD               # FAST_RED switch-over: h = 48 | 49 at w = 4, 9 | 14 at w = 14
assert (19 * 4 + 1) * FLD <= KW_FLOATS < (20 * 4 + 1) * FLD and (5 * 14 + 1) * FLD <= KW_FLOATS < (6 * 14 + 1) * FLD   # KW_FLOATS switch-over: h = 19 | 20, 5 | 6


def limit_grids():
    """The fall-back and limit grids, from the restated formulas: dict name -> (h, w)."""
    out = {}
    for w in (4, 14):
        for bwd in (False, True):
            d = "bwd" if bwd else "fwd"
            hf, ha = largest_h(w, bwd, True), largest_h(w, bwd, False)
            out[f"{d} w={w} last fast"] = (hf, w)
            if ha > hf:
                out[f"{d} w={w} first per-pixel"] = (hf + 1, w)
                out[f"{d} w={w} last accepted"] = (ha, w)
            out[f"{d} w={w} first refused"] = (ha + 1, w)
    return out


Case = namedtuple("Case", "dtype variant kind B h w p seed")


def branch_cases(grids, dtypes, B=2):
    """Per grid and dtype: the four variants with every parameter random, and the hybrid with a zero projector.  The three dropout cases rotate
    over grids, variants and dtypes, so that every variant and dtype meets each of them."""
    out = []
    for gi, (h, w) in enumerate(grids):
        for di, dt in enumerate(dtypes):
            out += [Case(dt, v, "A", B, h, w, *DROPS[(gi + vi + di) % 3]) for vi, v in enumerate(VARIANTS)]
            out.append(Case(dt, "hybrid", "Z", B, h, w, *DROPS[(gi + di + 1) % 3]))
    return out


def hybrid_cases(grids, dtype, B=2):
    return [Case(dtype, "hybrid", "A", B, h, w, *DROPS[i % 3]) for i, (h, w) in enumerate(grids)]


PIXEL_CASES = branch_cases(PIXEL_GRIDS, (BF16, F32)) + branch_cases(PIXEL_GRIDS_FP32, (F32,))
FAST4_CASES = branch_cases([(h, 4) for h in FAST_H_W4], (BF16,))
FAST14_CASES = branch_cases([(h, 14) for h in FAST_H_W14], (BF16,))
IMAGE_SUM_CASES = [Case(BF16, "hybrid", "A", B, 1, 4, *DROPS[i % 3]) for i, B in enumerate(IMAGE_SUM_B)] + \
                  [Case(F32, "hybrid", "A", B, 1, 3, *DROPS[(i + 1) % 3]) for i, B in enumerate(IMAGE_SUM_B)]
ATOMIC_CASES = [Case(BF16, "hybrid", "A", 17, 1, 4, *DROPS[1]), Case(F32, "hybrid", "A", 17, 2, 3, *DROPS[2]), Case(BF16, "noise_aware", "A", 17, 2, 3, *DROPS[0])]


def limit_cases(bwd):
    """Hybrid, bf16 and fp32, at the accepted grids of limit_grids() for one direction."""
    d = "bwd" if bwd else "fwd"
    grids = sorted({g for k, g in limit_grids().items() if k.startswith(d) and "refused" not in k})
    return hybrid_cases(grids, BF16) + hybrid_cases(grids[-2:], F32)


def refused_grids(bwd):
    d = "bwd" if bwd else "fwd"
    return sorted({g for k, g in limit_grids().items() if k.startswith(d) and "refused" in k})


def all_spatial_cases():
    return PIXEL_CASES + FAST4_CASES + FAST14_CASES + IMAGE_SUM_CASES + ATOMIC_CASES + limit_cases(False) + limit_cases(True)


_PARAMS = {}


def case_inputs(case):
    """(t, dd, P, keep) of a case: t, dd rounded to its dtype; P fp32; keep uint8 or None."""
    key = (case.variant, case.kind)
    if key not in _PARAMS:
        _PARAMS[key] = spatial_params(case.variant, case.kind)
    t, dd = spatial_operands(case.B, case.h, case.w, case.dtype, 100 * case.h + case.w + 7 * case.B)
    return t, dd, _PARAMS[key], keep_mask(case.B, 1 + case.h * case.w, case.p, case.seed)


def case_name(case):
    return f"{str(case.dtype).replace('torch.', '')} {case.variant}/{case.kind} B={case.B} {case.h}x{case.w} p={case.p}"


PRE_D = (4, 64, 256, 260, 768, 772, 1024)
PRE_D_REFUSED = (6, 1028)
PRE_M = (1, 3, 4, 5)
PRE_LONG = ((8197, 64), (8197, 260))
assert [pre_nv(D) for D in PRE_D] == [1, 1, 1, 3, 3, 4, 4] and not any(pre_accepted(1, D) for D in PRE_D_REFUSED)
assert all(M > 4 * PRE_GRID_CAP and M % (4 * PRE_GRID_CAP) for M, _ in PRE_LONG)
EPS = 1e-5


def pre_operands(M, D, dtype, seed, mean=0.0):
    x = rnd(M, D, seed=3000 + seed, shift=mean)
    du = rnd(M, D, seed=4000 + seed).to(dtype)
    dy = rnd(M, D, seed=5000 + seed)
    nw, nb = rnd(D, seed=6000 + seed, scale=0.3, shift=1.0), rnd(D, seed=6100 + seed, scale=0.3)
    gamma, gammax = rnd(D, seed=6200 + seed, scale=0.3), rnd(D, seed=6300 + seed, scale=0.3, shift=1.0)
    return x, du, dy, nw, nb, gamma, gammax


# ------------------------------------------------------------------------------------------ the spatial operator
def _frame7(k, n):
    """[64, n·n] taps in the 7 × 7 frame."""
    out = torch.zeros(BOTT, 7, 7, dtype=F64)
    o = (7 - n) // 2
    out[:, o:o + n, o:o + n] = k.to(F64).reshape(BOTT, n, n)
    return out


def _stencil(img, k7, flip=False, stray=None):
    """k7 [64, 7, 7], or [B, 64, 7, 7] per image.  out[b, y, x, c] = Σ_ij k7[c, i, j]·img[b, y + i − 3, x + j − 3, c], zero outside the grid (flip: y − (i − 3), x − (j − 3): the transposed
    stencil).  stray = (i, j, value [B, 64]): that tap reads `value` outside the grid (a planted bug)."""
    B, h, w, C = img.shape
    xp = torch.zeros(B, h + 6, w + 6, C, dtype=F64)
    xp[:, 3:3 + h, 3:3 + w] = img
    out = torch.zeros_like(img)
    for i in range(7):
        for j in range(7):
            a, b = (6 - i, 6 - j) if flip else (i, j)
            src = xp[:, a:a + h, b:b + w]
            if stray is not None and (i, j) == stray[:2]:
                inside = torch.zeros(h + 6, w + 6, dtype=torch.bool)
                inside[3:3 + h, 3:3 + w] = True
                src = torch.where(inside[a:a + h, b:b + w][None, :, :, None], src, stray[2][:, None, None, :])
            k = k7[..., i, j]
            out += (k[:, None, None, :] if k.dim() == 2 else k) * src
    return out


def _taps(dc, t_img):
    """dK[c, i, j] per image = Σ_yx dc[b, y, x, c]·t[b, y + i − 3, x + j − 3, c]: [B, 64, 7, 7]."""
    B, h, w, C = dc.shape
    xp = torch.zeros(B, h + 6, w + 6, C, dtype=F64)
    xp[:, 3:3 + h, 3:3 + w] = t_img
    out = torch.zeros(B, C, 7, 7, dtype=F64)
    for i in range(7):
        for j in range(7):
            out[:, :, i, j] = (dc * xp[:, i:i + h, j:j + w]).sum((1, 2))
    return out


class Err:
    """The three error channels of a tensor, all non-negative: e, fp32 roundings in units of u; a, absolute (the GELU approximation); mf, Σ|a||b| of the
    bf16 matrix-core products behind it (times u_mfma in the bound).  A later stage maps each channel through its absolute values (lin); the stage's own
    roundings add count·Σ|terms| to e (own), its own matrix-core product Σ|a||b| to mf (own_mf)."""

    def __init__(self, e, a=None, mf=None):
        self.ch = [e, torch.zeros_like(e) if a is None else a, torch.zeros_like(e) if mf is None else mf]

    e = property(lambda self: self.ch[0])
    mf = property(lambda self: self.ch[2])

    def lin(self, fn):
        return Err(*[fn(x) for x in self.ch])

    def __add__(self, other):
        return Err(*[x + y for x, y in zip(self.ch, other.ch)])

    def own(self, count, terms):
        return Err(self.ch[0] + count * terms, self.ch[1], self.ch[2])

    def own_mf(self, terms):
        return Err(self.ch[0], self.ch[1], self.ch[2] + terms)

    def term(self, ref):
        return Term(ref, *self.ch)


def _forward(variant, t, P, h, w, bug=None):
    """The forward stages on float64 t [B, 1 + hw, 64], each with its error channels; everything the backward needs."""
    B = t.shape[0]
    hw = h * w
    P = {k: v.to(F64) for k, v in P.items()}
    gh, gw = (w, h) if bug == "hw_swapped" else (h, w)
    tc, ts = t[:, 0], t[:, 1:].reshape(B, gh, gw, BOTT)
    f = P["freq"] if has_freq(variant) else torch.ones(BOTT, dtype=F64)
    K = [_frame7(P["conv1_w"], 3), _frame7(P["conv2_w"], 5), _frame7(P["conv3_w"], 7)]
    bias = [P["conv1_b"], P["conv2_b"], P["conv3_b"]]
    stray = (3, 2, tc) if bug == "border_tap" else None
    conv = [f * _stencil(ts, k, stray=stray) + b for k, b in zip(K, bias)]                    # conv_k = f·(k_k ⋆ t) + b_k
    e_conv = [N_CONV * (f.abs() * _stencil(ts.abs(), k.abs()) + b.abs()) for k, b in zip(K, bias)]
    st = dict(B=B, h=gh, w=gw, hw=hw, f=f, K=K, conv=conv, e_conv=e_conv, tc=tc, ts=ts, P=P)
    if has_noise(variant):
        n1, n3 = P["ne1_w"], P["ne3_w"]
        pool = f * ts.mean((1, 2))                                                           # [B, 64]
        e_pool = n_pool(hw) * f.abs() * ts.abs().mean((1, 2))
        hpre = pool @ n1.T + P["ne1_b"]                                                      # [B, 16]
        e_hid = e_pool @ n1.abs().T + N_NE1 * (pool.abs() @ n1.abs().T + P["ne1_b"].abs())   # ReLU passes an error on at most unchanged
        hid = hpre.clamp_min(0)
        logit = hid @ n3.T + P["ne3_b"]                                                      # [B, 3]
        e_logit = e_hid @ n3.abs().T + N_NE3 * (hid @ n3.abs().T + P["ne3_b"].abs())
        wts = torch.softmax(logit, 1)
        if bug == "weights_exchanged":
            wts = wts[:, [2, 1, 0]]
        relw = 2 * e_logit.amax(1) + N_SOFTMAX                                               # [B]: each weight's relative error, in units of u
        st.update(pool=pool, e_pool=e_pool, hpre=hpre, hid=hid, e_hid=e_hid)
    else:
        wts = torch.full((B, 3), 1.0 / 3.0, dtype=F64)
        relw = torch.full((B,), float(N_THIRD), dtype=F64)
    wv = wts[:, None, None, :, None]                                                         # [B, 1, 1, 3, 1]
    mix = (torch.stack(conv, 3) * wv).sum(3)
    e_mix = (torch.stack(e_conv, 3) * wv).sum(3) + relw[:, None, None, None] * (torch.stack(conv, 3).abs() * wv).sum(3)
    ident = f * ts if bug == "identity_filtered" else ts
    c = mix + ident
    e_c = e_mix + N_IDENT * (mix.abs() + ts.abs())
    if bug == "last_pixel":                       # the last pixel of the last pixel group never computed
        c = c.reshape(B, hw, BOTT).clone()
        c[:, hw - 1] = 0
        c = c.reshape(B, gh, gw, BOTT)
    Pw, pb = P["proj_w"], P["proj_b"]
    z_sp = c + c @ Pw.T + pb
    e_z = e_c + e_c @ Pw.abs().T + N_PROJ * (c.abs() + c.abs() @ Pw.abs().T + pb.abs())
    mf_z = c.abs() @ Pw.abs().T
    z_cls = tc
    if bug == "cls_through":
        z_cls = tc + tc @ Pw.T + pb
    with_cls = lambda v: torch.cat([torch.zeros(B, 1, BOTT, dtype=F64), v.reshape(B, hw, BOTT)], 1)                  # the CLS row is t itself: no error  # noqa: E731
    z = torch.cat([z_cls[:, None], z_sp.reshape(B, hw, BOTT)], 1)
    st.update(wts=wts, relw=relw, c=c, c_err=Err(e_c), z=z, z_err=Err(with_cls(e_z), None, with_cls(mf_z)))
    return st


def _scale(keep, p_drop, shape):
    if keep is None:
        return torch.ones(shape, dtype=F64)
    return keep.to(F64).reshape(shape) / (1.0 - float(torch.tensor(p_drop, dtype=F32)))


def spatial_fwd(variant, t, P, h, w, keep=None, p_drop=0.0, bug=None):
    """c (spatial tokens [B, hw, 64]), z and d ([B, 1 + hw, 64]) of uia_mona_spatial_fwd."""
    st = _forward(variant, t.to(F64), P, h, w, bug)
    B, hw, z, ez = st["B"], st["hw"], st["z"], st["z_err"]
    ks = _scale(keep, p_drop, z.shape)
    ed = Err(ks * (GP1 * ez.e + N_GELU * gelu(z).abs()), ks * z.abs() * A_PHI, ks * GP1 * ez.mf)
    return dict(c=st["c_err"].lin(lambda v: v.reshape(B, hw, BOTT)).term(st["c"].reshape(B, hw, BOTT)), z=ez.term(z), d=ed.term(gelu(z) * ks))


def spatial_bwd(variant, t, dd, P, h, w, keep=None, p_drop=0.0, bug=None):
    """dt [B, 1 + hw, 64] and every adapter_conv gradient of uia_mona_spatial_bwd, summed over the images: dict keyed dt, g_<parameter>."""
    t, dd = t.to(F64), dd.to(F64)
    st = _forward(variant, t, P, h, w, bug)
    B, hw, gh, gw, f, K, Pq = st["B"], st["hw"], st["h"], st["w"], st["f"], st["K"], st["P"]
    Pw, aP, fa = Pq["proj_w"], Pq["proj_w"].abs(), f.abs()
    z, ez = st["z"], st["z_err"]
    ks = _scale(keep, p_drop, z.shape)
    g = (dd * ks).abs()
    dz_all = dd * ks * dgelu(z)
    edz_all = Err(g * (GP2 * ez.e + N_GELU * dgelu(z).abs()), g * A_DPHI, g * GP2 * ez.mf)
    nb = B - 1 if bug == "last_image" else B          # images that reach a parameter gradient
    ni = n_img(B)
    grid = lambda v: v[:, 1:].reshape(B, gh, gw, BOTT)                                                                # noqa: E731
    flat = lambda v: v.reshape(B, hw, BOTT)                                                                           # noqa: E731
    pair = lambda a, b: torch.einsum("bpo,bpi->boi", flat(a)[:nb], flat(b)[:nb]).sum(0)       # Σ_b Σ_px a[px, co]·b[px, ci]       # noqa: E731
    tot = lambda v: flat(v)[:nb].sum((0, 1))                                                                          # noqa: E731
    dz, edz = grid(dz_all), edz_all.lin(grid)
    c, ec = st["c"], st["c_err"]
    out = {}
    # dP = Σ dz·c (matrix cores in the fast kernel), db_p = Σ dz
    terms = pair(dz.abs(), c.abs())
    out["g_proj_w"] = (edz.lin(lambda v: pair(v, c.abs())) + ec.lin(lambda v: pair(dz.abs(), v))).own(hw + ni, terms).own_mf(terms).term(pair(dz, c))
    out["g_proj_b"] = edz.lin(tot).own(hw + ni, tot(dz.abs())).term(tot(dz))
    # dc = dz + Pᵀ·dz
    dc = dz + dz @ Pw
    edc = (edz + edz.lin(lambda v: v @ aP)).own(N_DC, dz.abs() + dz.abs() @ aP).own_mf(dz.abs() @ aP)
    wts, relw = st["wts"], st["relw"]
    ts, ats = st["ts"], st["ts"].abs()
    # pass A: dK per image (hw summands), then g_conv_k_w = Σ_b w_k·f·dK (restricted to the sub-stencil), g_conv_k_b = Σ_b w_k·Σ_px dc
    dk, dk_abs = _taps(dc, ts), _taps(dc.abs(), ats)
    edk = edc.lin(lambda v: _taps(v, ats)).own(hw, dk_abs)
    sdc, sdc_abs = dc.sum((1, 2)), dc.abs().sum((1, 2))                                        # [B, 64]
    esdc = edc.lin(lambda v: v.sum((1, 2))).own(hw, sdc_abs)
    for k, n in enumerate((3, 5, 7)):
        o = (7 - n) // 2
        wk = wts[:, k]
        cut = lambda v: v[:, :, o:o + n, o:o + n].reshape(B, BOTT, n * n)                                              # noqa: E731
        scale = lambda v: wk[:, None, None] * fa[None, :, None] * cut(v)                                               # noqa: E731
        per = scale(dk_abs)
        e = edk.lin(lambda v: scale(v)[:nb].sum(0)).own(1, ((N_DK_SCALE + relw)[:, None, None] * per)[:nb].sum(0)).own(ni, per[:nb].sum(0))
        out[f"g_conv{k + 1}_w"] = e.term((wk[:, None, None] * f[None, :, None] * cut(dk))[:nb].sum(0))
        per = wk[:, None] * sdc_abs
        e = esdc.lin(lambda v: (wk[:, None] * v)[:nb].sum(0)).own(1, ((1 + relw)[:, None] * per)[:nb].sum(0)).own(ni, per[:nb].sum(0))
        out[f"g_conv{k + 1}_b"] = e.term((wk[:, None] * sdc)[:nb].sum(0))
    dpool, dpool_abs, edpool = torch.zeros(B, BOTT, dtype=F64), torch.zeros(B, BOTT, dtype=F64), Err(torch.zeros(B, BOTT, dtype=F64))
    if has_noise(variant):
        # dw_k = Σ_{c, px} dc·conv_k;  softmax backward;  hidden layer behind its gate;  the pool
        conv, e_conv = st["conv"], st["e_conv"]
        over = lambda fn: torch.stack([fn(k).sum((1, 2, 3)) for k in range(3)], 1)             # [B, 3]                 # noqa: E731
        cabs = [e / N_CONV for e in e_conv]                 # |f|·(|k_k| ⋆ |t|) + |b_k|: the fast kernel forms Σ dc·conv_k from the taps of dK, whose errors meet |k_k| ⋆ |t|, not |conv_k|
        dwm, dwm_abs = over(lambda k: dc * conv[k]), over(lambda k: dc.abs() * cabs[k])
        edwm = (edc.lin(lambda v: over(lambda k: v * cabs[k])) + Err(over(lambda k: dc.abs() * e_conv[k]))).own(hw + N_DWM, dwm_abs)
        dl = wts * (dwm - (dwm * wts).sum(1, keepdim=True))
        spread = lambda v: wts * (v + (v * wts).sum(1, keepdim=True))                                                  # noqa: E731
        dl_abs = spread(dwm_abs)
        edl = edwm.lin(spread).own(1, (2 * relw + N_DL)[:, None] * dl_abs)                      # the weights' own error: w_k and the w_j inside dot
        gate = torch.ones_like(st["hpre"]) if bug == "relu_gate" else (st["hpre"] > 0).to(F64)
        n1, n3 = Pq["ne1_w"], Pq["ne3_w"]
        dh, dh_abs = (dl @ n3) * gate, (dl.abs() @ n3.abs()) * gate                            # [B, 16]
        edh = edl.lin(lambda v: (v @ n3.abs()) * gate).own(N_DH, dh_abs)
        outer = lambda a, b: torch.einsum("bk,bj->kj", a[:nb], b[:nb])                                                 # noqa: E731
        col = lambda v: v[:nb].sum(0)                                                                                  # noqa: E731
        hid, pool = st["hid"], st["pool"]
        out["g_ne3_w"] = (edl.lin(lambda v: outer(v, hid)) + Err(outer(dl.abs(), st["e_hid"]))).own(1 + ni, outer(dl.abs(), hid)).term(outer(dl, hid))
        out["g_ne3_b"] = edl.lin(col).own(ni, col(dl.abs())).term(col(dl))
        out["g_ne1_w"] = (edh.lin(lambda v: outer(v, pool.abs())) + Err(outer(dh.abs(), st["e_pool"]))).own(1 + ni, outer(dh.abs(), pool.abs())).term(outer(dh, pool))
        out["g_ne1_b"] = edh.lin(col).own(ni, col(dh.abs())).term(col(dh))
        if bug != "pool_gradient":
            dpool, dpool_abs = dh @ n1 / hw, dh.abs() @ n1.abs() / hw                          # [B, 64]
            edpool = edh.lin(lambda v: v @ n1.abs() / hw).own(N_DPOOL, dpool_abs)
    # pass B: dxf = Kᵀ ⋆ dc + dpool;  dt = dc + f·dxf;  df = Σ dxf·t
    km = sum(wts[:, k, None, None, None] * K[k] for k in range(3))                             # [B, 64, 7, 7]
    km_abs = sum(wts[:, k, None, None, None] * K[k].abs() for k in range(3))
    acc, acc_abs = _stencil(dc, km, flip=True), _stencil(dc.abs(), km_abs, flip=True)
    wide = lambda v: v[:, None, None, :]                                                                              # noqa: E731
    dxf, dxf_abs = acc + wide(dpool), acc_abs + wide(dpool_abs)
    edxf = (edc.lin(lambda v: _stencil(v, km_abs, flip=True)) + edpool.lin(wide)).own(1, (N_DXF + relw)[:, None, None, None] * acc_abs + dxf_abs)
    edt = (edc + edxf.lin(lambda v: fa * v)).own(N_DT, dc.abs() + fa * dxf_abs)
    cls = dz_all[:, :1]
    if bug == "cls_through":
        cls = cls + cls @ Pw
    ecls = edz_all.lin(lambda v: v[:, :1])
    out["dt"] = Err(*[torch.cat([a, flat(b)], 1) for a, b in zip(ecls.ch, edt.ch)]).term(torch.cat([cls, flat(dc + f * dxf)], 1))
    if has_freq(variant):
        red = lambda v: v[:nb].sum((0, 1, 2))                                                                          # noqa: E731
        out["g_freq"] = edxf.lin(lambda v: red(v * ats)).own(hw + ni, red(dxf_abs * ats)).term(red(dxf * ts))
    return out


def bound(term, count=1, dtype=F32, fast=False, prefill=None):
    """C·u·mag + a + u_mfma·mf (fast kernel only) + u_out·|ref|.  The spatial terms carry their counts inside mag (count = 1); the pre-norm terms take
    C_U, C_DX or c_pre_sum.  prefill: the values an accumulating output held before the launch."""
    import helpers_reference as R
    ref, mag = term.ref, term.mag
    if prefill is not None:
        ref, mag = ref + prefill.to(F64), mag + prefill.to(F64).abs()
    return count * U * mag + term.a + (U_MFMA * term.mf if fast else 0) + R.U_OUT[dtype] * ref.abs()


# ------------------------------------------------------------------------------------------ the pre-norm
def _stats(x, eps):
    M, D = x.shape
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xhat = (x - mu) * rstd
    a1 = x.abs().mean(1, keepdim=True)
    # the mean's error C_MEAN·u·a1 shifts every x̂ by rstd times it, and enters the variance at second order: (δ·rstd)²/2 relative on x̂
    xhat_mag = rstd * a1 + xhat.abs() * (1 + (C_MEAN * a1 * rstd) ** 2 * U / 2)
    return rstd, xhat, xhat_mag


def pre_fwd(x, nw, nb, gamma, gammax, eps=EPS):
    """u = (x̂·w + b)·γ + x·γx of uia_mona_pre_fwd."""
    x, nw, nb, gamma, gammax = (v.to(F64) for v in (x, nw, nb, gamma, gammax))
    rstd, xhat, xm = _stats(x, eps)
    ref = (xhat * nw + nb) * gamma + x * gammax
    mag = (xm * nw.abs() + nb.abs()) * gamma.abs() + (x * gammax).abs()
    z = torch.zeros_like(ref)
    return dict(u=Term(ref, mag, z, z))


def pre_rows_of_waves(M):
    """Rows each wave of the persistent grid walks (grid at its cap, before the occupancy cut): list of row lists."""
    grid = pre_grid_cap(M)
    return [list(range(blk * 4 + wv, M, 4 * grid)) for blk in range(grid) for wv in range(4)]


def pre_bwd(du, x, dy, nw, nb, gamma, gammax, eps=EPS, bug=None):
    """dx = dy + du·γx + LN'(du·γ·w) (None without dy) and dγ, dγx, dw_n, db_n of uia_mona_pre_bwd."""
    du, x, nw, nb, gamma, gammax = (v.to(F64) for v in (du, x, nw, nb, gamma, gammax))
    M, D = x.shape
    rstd, xhat, xm = _stats(x, eps)
    out = {}
    zero = torch.zeros(D, dtype=F64)
    if dy is not None:
        dy = dy.to(F64)
        gv = du * gamma * nw
        ref = dy + du * gammax + rstd * (gv - gv.mean(1, keepdim=True) - xhat * (gv * xhat).mean(1, keepdim=True))
        # x̂·mean(g·x̂) by the product rule, an error of x̂ (xm) on one factor at a time: with rows far from zero xm is many times |x̂|, and
        # xm·mean(|g|·xm) would let the bound grow with the square of the row's mean
        mag = dy.abs() + (du * gammax).abs() + rstd * (gv.abs() + gv.abs().mean(1, keepdim=True) + xm * (gv * xhat).abs().mean(1, keepdim=True)
                                                       + xhat.abs() * (gv.abs() * xm).mean(1, keepdim=True))
        out["dx"] = Term(ref, mag, torch.zeros_like(ref), torch.zeros_like(ref))
    rows = torch.ones(M, 1, dtype=F64)
    if bug == "odd_wave_row":                     # a wave that walks an odd number of rows loses its last one
        for r in pre_rows_of_waves(M):
            if len(r) % 2:
                rows[r[-1]] = 0
    S0, S1, S2 = (du * rows).sum(0), (du * xhat * rows).sum(0), (du * x * rows).sum(0)
    m0, m1, m2 = du.abs().sum(0), (du.abs() * xm).sum(0), (du * x).abs().sum(0)
    out["g_gamma"] = Term(nw * S1 + (0 if bug == "dgamma_s1" else nb * S0), nw.abs() * m1 + nb.abs() * m0, zero, zero)
    out["g_gammax"] = Term(S2, m2, zero, zero)
    out["g_nw"] = Term(gamma * S1, gamma.abs() * m1, zero, zero)
    out["g_nb"] = Term(gamma * S0, gamma.abs() * m0, zero, zero)
    return out


def pre_count(name, M):
    return dict(u=C_U, dx=C_DX).get(name) or c_pre_sum(M)


def kb_layout(dx, kb_rows, dtype, bug=None):
    """The K-blocked copy of a row-major [M, D] tensor: [D/g, kb_rows, g] with g = 64 bytes of elements, rows M .. kb_rows NaN (untouched)."""
    M, D = dx.shape
    g = 64 // torch.empty(0, dtype=dtype).element_size()
    out = torch.full((D // g, kb_rows, g), float("nan"), dtype=dx.dtype)
    blocks = dx.reshape(M, D // g, g).permute(1, 0, 2)
    if bug == "kb_offset":
        blocks = blocks.roll(1, 0)
    out[:, :M] = blocks
    return out
