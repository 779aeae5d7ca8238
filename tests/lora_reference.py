"""The LoRA dropout generator restated on the host, float64 restatements of the kernels that apply or regenerate it, and the bounds
that judge them.

A plain module, no pytest: tests/test_lora_contract_gpu.py runs uia_dropout, the N = 64 / K = 64 stream GEMMs, the run-time GEMM
epilogue, uia_wgrad / _ex / _drop / _group, uia_lora_rank_update and uia_ln_lora_down next to these functions;
tests/test_lora_reference_host.py checks the generator against a scalar second form and its statistics, each restatement against
a second independent form, and shows that the bounds catch planted bugs on the CPU.

Generator (csrc/uia_common.h).  uia_hash32, dropout_thresh16, dropout_keep8 and the per-element dropout_keep of the Mona kernels
are restated with numpy uint64 arithmetic masked to 32 bits.  Two quantisations are part of the contract: the drop probability is
quantised to thresh16 / 65536 (thresh16 = floor(p·65536 + 0.5) in fp32, clamped to 65535), and the kept values scale by the fp32
quotient 1 / (1 − p) of the UNQUANTISED p.

Every float64 reference takes CPU tensors holding exactly the operands the kernel sees and returns (ref, mag), mag being the sum
of the absolute values of the terms of each element.  Bounds as in tests/helpers_reference.py:
|k − ref| ≤ C·u·mag + u_out·|ref|, u = 2^-24.  The dropped operand bf16(fp32(x)·fp32(1/(1−p))) is reproduced bit for bit
(one fp32 product, one rounding), so kept sets, dropped operands and untouched elements are compared exactly.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from helpers_reference import F64, U, U_OUT, Checker, bound  # noqa: F401  (re-exported for the tests)

M32 = np.uint64(0xFFFFFFFF)
M64 = 0xFFFFFFFFFFFFFFFF

# ---- calibrated constants.  Each is about twice the worst error-to-bound ratio measured on the MI355X with the constant set to 1,
#      over every comparison of test_lora_contract_gpu.py that uses it (worst measured in the comment).  A bf16 result's own rounding
#      (u_out·|ref|) fills the bound to 0.99 on its own at a value just above a power of two: those bars say that the fp32 arithmetic
#      underneath stays invisible below it, the fp32 bars (out32, the weight gradients) measure that arithmetic itself.
C_GEMM_DROP_A = 2.0     # N = 64 stream GEMM, t = drop(a)·wᵀ + bias (bf16 t)   measured 0.995
C_GEMM_DROP_ACC = 2.0   # K = 64 stream GEMM / run-time epilogue, resid + drop(alpha·a·wᵀ + bias)   measured run-time epilogue fp32 1.00, bf16 0.991;
                        #   cfg 23 fp32 0.793, bf16 0.988
C_WGRAD = 2.5           # uia_wgrad / _ex / _drop / _group dW   measured fp32 plain 1.26, ex 1.14; bf16 drop 0.906, group 0.878
C_WGRAD_BIAS = 1.5      # ... dbias   measured fp32 0.757 (plain), 0.618 (ex); bf16 group 0.496
C_RANK = 2.0            # uia_lora_rank_update (bf16 out, in place)   measured 0.996 (also with waves walking 2, 3 and 4 units)
C_LN_H = 2.0            # uia_ln_lora_down h (bf16)   measured 0.996, rows of mean 100 included
C_LN_T = 2.0            # uia_ln_lora_down t (bf16)   measured 0.996


# ------------------------------------------------------------------------------------------ the generator
def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def hash32(x):
    """uia_hash32 on an array of 32-bit values held in uint64."""
    x = _u64(x) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def thresh16(p):
    """dropout_thresh16: t = p·65536 + 0.5 in fp32 (one product — exact, a power of two — and one rounded sum); 0 below 0, 65535 from
    65535 on, else truncated."""
    t = np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5)
    if t <= np.float32(0.0):
        return 0
    if t >= np.float32(65535.0):
        return 65535
    return int(t)


def keep_rate(p):
    """The keep probability the generator realises: 1 − thresh16 / 65536."""
    return 1.0 - thresh16(p) / 65536.0


def inv_keep32(p):
    """fp32 1 / (1 − p), as the launchers and kernels compute it (correctly rounded subtraction and division)."""
    one = np.float32(1.0)
    return np.float32(one / np.float32(one - np.float32(p)))


def keep8(seed, grp, th16):
    """dropout_keep8 for an array of group indices: [G, 8] bool, column e = keep element 8·grp + e.  One hash of a hash, then three
    xorshift32 steps; the low half of each word decides the even element, the high half the odd one."""
    seed = int(seed) & M64
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    grp = _u64(grp).reshape(-1) & M32
    h = hash32((hash32(grp ^ lo) + hi) & M32)
    th = np.uint64(th16)
    out = np.empty((grp.size, 8), dtype=bool)
    for q in range(4):
        out[:, 2 * q] = (h & np.uint64(0xFFFF)) >= th
        out[:, 2 * q + 1] = (h >> np.uint64(16)) >= th
        h = h ^ ((h << np.uint64(13)) & M32)
        h = h ^ (h >> np.uint64(17))
        h = h ^ ((h << np.uint64(5)) & M32)
    return out


def mona_thresh(p):
    """The Mona kernels' 32-bit threshold: min(p·2^32, 2^32 − 1) in fp32, truncated (2^32 − 1 rounds to 2^32 in fp32; the
    conversion saturates); 0 when p is 0."""
    if not p > 0:
        return 0
    t = np.float32(np.float32(p) * np.float32(4294967296.0))
    return int(min(float(t), 4294967295.0))


def keep_elem(seed, idx, thresh):
    """dropout_keep (per element; the Mona kernels): bool array."""
    seed = int(seed) & M64
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    idx = _u64(idx).reshape(-1) & M32
    h = hash32(idx ^ lo) ^ hash32(((idx * np.uint64(0x9E3779B9)) & M32) + hi)
    return hash32(h) >= np.uint64(thresh)


def keep_mask(seed, rows, width, p, ld=None, col0=0):
    """bool [rows, width] tensor: the mask uia_dropout draws for a row-major tensor of `ld` (default `width`) columns, restricted to the
    `width` columns from col0 on (uia_wgrad_drop's window).  width, ld and col0 are multiples of 8."""
    ld = width if ld is None else ld
    assert width % 8 == 0 and ld % 8 == 0 and col0 % 8 == 0 and col0 + width <= ld
    r = np.arange(rows, dtype=np.uint64)[:, None]
    g = np.arange(width // 8, dtype=np.uint64)[None, :]
    grp = (r * np.uint64(ld) + np.uint64(col0)) // np.uint64(8) + g
    return torch.from_numpy(keep8(seed, grp, thresh16(p)).reshape(rows, width))


def mona_keep_mask(seed, shape, p):
    """uint8 tensor of `shape`: the per-element mask of the Mona kernels over the flat element index."""
    n = math.prod(shape)
    return torch.from_numpy(keep_elem(seed, np.arange(n, dtype=np.uint64), mona_thresh(p)).astype(np.uint8)).reshape(shape)


def derived_seeds(base, n):
    """The seeds functional._next_seed hands out for calls 1..n after set_dropout_seed(base)."""
    return [(base * 0x9E3779B97F4A7C15 + c * 0xD1B54A32D192ED03) & M64 for c in range(1, n + 1)]


EDGE_SEEDS = (0, 1, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1)
SEEDS = EDGE_SEEDS + tuple(derived_seeds(0x5EED, 4))


# ------------------------------------------------------------------------------------------ exact pieces
def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded, from float64: a·b is exact in float64 (48 bits); the sum is taken with its rounding error
    (TwoSum), and where the float64 sum sits exactly between two fp32 values the error decides the direction."""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    d = r.astype(np.float64) - s
    up = (err > 0) & (d < 0) & (np.abs(d) * 2 == np.abs(np.spacing(r).astype(np.float64)))
    dn = (err < 0) & (d > 0) & (np.abs(d) * 2 == np.abs(np.spacing(r).astype(np.float64)))
    r = np.where(up, np.nextafter(r, np.float32(np.inf)), r)
    r = np.where(dn, np.nextafter(r, np.float32(-np.inf)), r)
    return r.astype(np.float32)


def dropped(x, p, keep):
    """The dropped operand in x's dtype: keep ? T(fp32(x)·fp32(1/(1−p))) : 0 — one fp32 product, one rounding."""
    v = x.float() * torch.tensor(float(inv_keep32(p)), dtype=torch.float32)
    return torch.where(keep, v, torch.zeros_like(v)).to(x.dtype)


def dropout(src, p, seed, accumulate=False, dst0=None, keep=None):
    """uia_dropout on a flat tensor, exact: T(fma(src, keep·inv, accumulate ? dst0 : 0)) — the kernel's one fused multiply-add in fp32,
    then the rounding of the store.  Returns (values in src's dtype, keep mask); `keep` = the mask of (seed, p) where the caller has it."""
    n = src.numel()
    keep = (keep_mask(seed, 1, n, p) if keep is None else keep).reshape(-1)
    k = np.where(keep.numpy(), inv_keep32(p), np.float32(0.0)).astype(np.float32)
    base = dst0.reshape(-1).float().numpy() if accumulate else np.zeros(n, dtype=np.float32)
    out = fma32(src.reshape(-1).float().numpy(), k, base)
    return torch.from_numpy(out).to(src.dtype).reshape(src.shape), keep.reshape(src.shape)


# ------------------------------------------------------------------------------------------ float64 references
def gemm_drop_a(a, w, bias, p, seed):
    """N = 64 stream GEMM with dropout on the A operand: a_drop = dropped(a) (exact, a's dtype), t = a_drop·wᵀ + bias.
    Returns ((t, a_drop), mag)."""
    M, K = a.shape
    ad = dropped(a, p, keep_mask(seed, M, K, p)) if p > 0 else a.clone()
    b = bias.to(F64) if bias is not None else torch.zeros(w.shape[0], dtype=F64)
    t = ad.to(F64) @ w.to(F64).T + b
    mag = ad.to(F64).abs() @ w.to(F64).abs().T + b.abs()
    return (t, ad), mag


def gemm_drop_acc(a, w, alpha, bias, p, seed, resid):
    """resid + drop(alpha·a·wᵀ + bias), the mask drawn for the [M, N] result; the kept values scale by the fp32 1/(1−p).
    Returns (ref, mag, keep)."""
    M, N = a.shape[0], w.shape[0]
    b = bias.to(F64) if bias is not None else torch.zeros(N, dtype=F64)
    v = alpha * (a.to(F64) @ w.to(F64).T) + b
    vm = abs(alpha) * (a.to(F64).abs() @ w.to(F64).abs().T) + b.abs()
    keep = keep_mask(seed, M, N, p) if p > 0 else torch.ones(M, N, dtype=torch.bool)
    s = float(inv_keep32(p)) if p > 0 else 1.0
    r = resid.to(F64) if resid is not None else torch.zeros(M, N, dtype=F64)
    z = torch.zeros_like(v)
    return r + torch.where(keep, v * s, z), r.abs() + torch.where(keep, vm * s, z), keep


def wgrad(a, b, alpha, dw0, i_valid=None, j_valid=None, drop=None, dbias0=None):
    """dw0 + alpha·aᵀ·drop(b) on the valid extent [i_valid, j_valid], and dbias0 + Σ_m a[m, :i_valid].  drop = (p, keep [M, J]) or None.
    Returns dict(dw, mag_dw, db, mag_db): mag_dw = |dw0| + |alpha|·|a|ᵀ·|drop(b)|."""
    I, J = a.shape[1], b.shape[1]
    iv, jv = i_valid or I, j_valid or J
    bd = dropped(b, drop[0], drop[1]) if drop is not None else b
    a64, b64 = a.to(F64)[:, :iv], bd.to(F64)[:, :jv]
    out = dict(dw=dw0.to(F64) + alpha * (a64.T @ b64), mag_dw=dw0.to(F64).abs() + abs(alpha) * (a64.abs().T @ b64.abs()), db=None, mag_db=None)
    if dbias0 is not None:
        out["db"] = dbias0.to(F64)[:iv] + a64.sum(0)
        out["mag_db"] = dbias0.to(F64)[:iv].abs() + a64.abs().sum(0)
    return out


def lora_rank_update(out0, qs, ws, alpha, p, keeps):
    """out0 + Σ_s keep_s ? alpha/(1−p)·q_s·w_sᵀ : 0.  qs [M, 64], ws [N, 64] per source; keeps: bool [M, N] per source (None: p = 0).
    Returns (ref, mag)."""
    s = alpha * (float(inv_keep32(p)) if p > 0 else 1.0)
    ref, mag = out0.to(F64).clone(), out0.to(F64).abs()
    for i, (q, w) in enumerate(zip(qs, ws)):
        v = s * (q.to(F64) @ w.to(F64).T)
        vm = abs(s) * (q.to(F64).abs() @ w.to(F64).abs().T)
        if p > 0:
            v, vm = torch.where(keeps[i], v, torch.zeros_like(v)), torch.where(keeps[i], vm, torch.zeros_like(vm))
        ref, mag = ref + v, mag + vm
    return ref, mag


def layernorm(x, gamma, beta, eps):
    """LayerNorm over the last dimension in float64, written out.  The terms of an element are x·rstd·γ, mean·rstd·γ and β:
    mag = (|x| + mean|x|)·rstd·|γ| + |β|, with mean|x| = Σ|x| / D the magnitude of the terms of the mean.  (The mean carries an absolute
    error of a few u·mean|x| into EVERY element of its row, however small x − mean is there: a bound relative to |xhat| would not hold
    where x is close to the mean of a row far from zero.)"""
    x, gamma, beta = x.to(F64), gamma.to(F64), beta.to(F64)
    mu = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xhat = (x - mu) * rstd
    return xhat * gamma + beta, (x.abs() + x.abs().mean(1, keepdim=True)) * rstd * gamma.abs() + beta.abs()


def ln_lora_down(x, gamma, beta, eps, h_kernel, a_rows, p, keeps):
    """(h, mag_h) = layernorm(x) and, per source, (t_s, mag_s) = drop_s(h_kernel)·a_s[:16]ᵀ from the kernel's own stored bf16 h — that
    separates the product from the LayerNorm.  a_rows: [>= 16, D] each; keeps: bool [M, D] per source (None: p = 0)."""
    h, mag_h = layernorm(x, gamma, beta, eps)
    ts = []
    for i, a in enumerate(a_rows):
        hd = dropped(h_kernel, p, keeps[i]) if p > 0 else h_kernel
        ts.append((hd.to(F64) @ a[:16].to(F64).T, hd.to(F64).abs() @ a[:16].to(F64).abs().T))
    return (h, mag_h), ts


# ------------------------------------------------------------------------------------------ second forms (host test)
def layernorm_torch(x, gamma, beta, eps):
    return F.layer_norm(x.to(F64), (x.shape[1],), gamma.to(F64), beta.to(F64), eps)


# ------------------------------------------------------------------------------------------ case shapes shared by the GPU and host tests
DROPOUT_N = (8, 8 * 257, 8 * 65537)
DROPOUT_P = (0.0, 1e-6, 0.1, 0.25, 0.5, 0.9, 0.99999)
GEMM_A_M, GEMM_A_K = (1, 17, 130), (64, 320, 768)           # K / 32 = 2, 10, 24 steps in groups of 8 in flight: 10 leaves a partial group
GEMM_ACC_M, GEMM_ACC_N = (1, 16, 33), (64, 256)
GEMM_ACC_TILED = (33, 256, 128)                             # M, N, K of the launch that plan_gemm routes to a tiled kernel's run-time epilogue
WGRAD_M = (1, 127, 128, 129, 512, 513, 4097)                # 16-row tiles, the 128-row slab, the 512-row chunk, the ninth chunk (second round of XCD slots)
WGRAD_IJ = ((64, 64), (128, 64), (64, 192))
WGRAD_VALID = (("full", (None, None)), ("rows16", (16, None)), ("cols16", (None, 16)), ("5x7", (5, 7)))
RANK_M, RANK_N = (1, 15, 16, 17, 517), (256, 1024)
LN_D, LN_RANK, LN_M = (768, 1024), (1, 8, 16), (1, 15, 16, 17, 100)


def rank_walk_rows(ncu, N, k):
    """Smallest M at which some wave of lora_rank_update_kernel walks k units (launch_rank: 4·per_q workgroups, per_q = min(⌈units/8⌉,
    ncu/4); the eight waves of a column quarter's workgroups step by 8·per_q over its ⌈M/16⌉·N/256 units; wave 0 walks k of them once
    there are more than (k − 1)·8·per_q)."""
    nch = N // 256
    per_q = max(1, ncu // 4)
    ntiles = ((k - 1) * 8 * per_q) // nch + 1
    M = 16 * (ntiles - 1) + 1
    assert (-(-M // 16) * nch + 7) // 8 >= per_q            # the cap on per_q is what holds at this size
    return M


def ln_tiles_rows(ncu, per_cu):
    """Smallest M of uia_ln_lora_down with more 16-row tiles than a launch of per_cu·ncu workgroups has blocks."""
    return 16 * per_cu * ncu + 1
