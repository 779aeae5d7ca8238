// cls_grad.hip — the backward of the last image block and its adapter when the gradient is CLS-sparse.
//
// The contrastive head reads token 0 of every image only, so the gradient that enters the last adapter and the MLP half of the last block is
// non-zero in one row of every 1 + h·w.  Those stages work row by row and run on the B CLS rows through the ordinary launches; what is
// left for this file is the three places where the sparse rows meet a dense tensor:
//   attn_bwd_cls_kernel   attention backward with ONE non-zero query row per head; writes the whole dense dq / dk / dv
//   mona_cls_bwd_kernel   the adapter's dropout · GELU' on the CLS token (it bypasses the spatial operator), mask index of the DENSE tensor
//   copy_rows_kernel      rows of any 16-byte-granular type out of a strided tensor (row b·N of a saved activation)
// and their forward twins, for a tower whose caller reads token 0 of the last layer and nothing else (the last layer then runs on B rows):
//   attn_fwd_cls_kernel   attention forward of the ONE query row token 0 per head; compact out [B, H·64] and lse [B, H]
//   mona_cls_fwd_kernel   the adapter's dropout · GELU on the CLS token, mask index of the DENSE tensor
//   rows3_kernel          fp32 rows b·N of a three-byte tensor (bf16 hi plane, row-major or K-blocked, + int8 low bytes)
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

// sum over the 8 lanes that share one key (lanes 8i .. 8i+7): inside a quad, the other quad of the half-row
__device__ __forceinline__ float sum8(float v) {
    v += uia_dpp_quad_xor1(v);
    v += uia_dpp_quad_xor2(v);
    v += uia_dpp_half_mirror(v);
    return v;
}

constexpr int ACL_THREADS = 256, ACL_KEYS = ACL_THREADS / 8;     // 32 keys per pass, 8 lanes x 8 elements per key row

// One workgroup per (batch, head).  Lane group g = tid / 8 owns key j = 32·pass + g, lane s = tid % 8 its elements 8s .. 8s+7:
//   P_j = exp(scale·q·k_j − lse)   dV_j = P_j·dO   δ = dO·O   dS_j = P_j(dO·v_j − δ)·scale   dK_j = dS_j·q   dQ_0 = Σ_j dS_j k_j   dQ_l = 0 (l > 0)
// q, O, dO, lse: the CLS row (token 0) of the head.  One pass over K and V, every element of dq / dk / dv written once with 16-byte stores.
template <typename T, bool KB>
__global__ __launch_bounds__(ACL_THREADS) void attn_bwd_cls_kernel(const UiaAttnParams p, const int compact) {
    __shared__ float red[ACL_KEYS][64];
    const int tid = threadIdx.x, s = tid & 7, g = tid >> 3;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H, L = p.L;
    const size_t row0 = (size_t)b * L;
    const int col = h * 64 + 8 * s;
    float q[8], o[8], dO[8];
    load8((const T*)p.q + row0 * p.ld_qkv + col, q);
    load8((const T*)p.dout + (size_t)b * p.lddo + col, dO);
    if (compact) load8((const T*)p.out + (size_t)b * p.ldo + col, o);      // out [B, H·64], lse [B, H]: what attn_fwd_cls_kernel left
    else if (KB && p.out_kb_rows) load8((const T*)p.out + ((size_t)(col >> 5) * (size_t)p.out_kb_rows + row0) * 32 + (col & 31), o);
    else load8((const T*)p.out + row0 * p.ldo + col, o);
    const float lse = p.lse[compact ? (size_t)b * p.H + h : ((size_t)b * p.H + h) * L];
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) dl = fmaf(dO[e], o[e], dl);
    const float delta = sum8(dl);
    float dq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dq[e] = 0.f;
    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = g; j < L; j += ACL_KEYS) {
        const size_t row = row0 + j;
        float k[8], v[8];
        load8((const T*)p.k + row * p.ld_qkv + col, k);
        load8((const T*)p.v + row * p.ld_qkv + col, v);
        float sc = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc = fmaf(q[e], k[e], sc);
            dp = fmaf(dO[e], v[e], dp);
        }
        sc = sum8(sc);
        dp = sum8(dp);
        const float P = __expf(fmaf(sc, p.scale, -lse));
        const float dS = P * (dp - delta) * p.scale;
        float dk[8], dv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            dk[e] = dS * q[e];
            dv[e] = P * dO[e];
            dq[e] = fmaf(dS, k[e], dq[e]);
        }
        if (KB && p.dqkv_kb_rows) {
            const size_t off = ((size_t)(col >> 5) * (size_t)p.dqkv_kb_rows + row) * 32 + (col & 31);
            store8((T*)p.dk + off, dk);
            store8((T*)p.dv + off, dv);
            if (j > 0) store8((T*)p.dq + off, zero);
        } else {
            const size_t off = row * p.ld_dqkv + col;
            store8((T*)p.dk + off, dk);
            store8((T*)p.dv + off, dv);
            if (j > 0) store8((T*)p.dq + off, zero);
        }
    }
    // dQ of the CLS row: the 32 key groups' partial sums through LDS, fixed order
#pragma unroll
    for (int e = 0; e < 8; ++e) red[g][8 * s + e] = dq[e];
    __syncthreads();
    if (tid < 8) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int r = 0; r < ACL_KEYS; ++r)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += red[r][8 * tid + e];
        const int c0 = h * 64 + 8 * tid;
        if (KB && p.dqkv_kb_rows) store8((T*)p.dq + ((size_t)(c0 >> 5) * (size_t)p.dqkv_kb_rows + row0) * 32 + (c0 & 31), acc);
        else store8((T*)p.dq + row0 * p.ld_dqkv + c0, acc);
    }
}

constexpr int ACL_MAX_L = 288, ACL_PASSES = ACL_MAX_L / ACL_KEYS;

// The forward twin: one workgroup per (batch, head), lane group g owns keys j = 32·pass + g < n (n = L, or max(keylen[b], 1) with key padding), q = token 0.
//   s_j = scale·q·k_j   m = max_j s_j   P_j = exp(s_j − m)   l = Σ_j P_j   O = Σ_j P_j v_j / l   lse = m + log l
// The scores of a lane group's (at most nine) keys stay in registers between the K pass and the V pass; no K or V row at or beyond n is read.
// O and l: the 32 key groups' partial sums through LDS, fixed order.  out [B, H·64] (row stride ldo), lse [B, H].
template <typename T, bool KEYPAD>
__global__ __launch_bounds__(ACL_THREADS) void attn_fwd_cls_kernel(const UiaAttnParams p) {
    __shared__ float red[ACL_KEYS][64];
    __shared__ float lred[ACL_KEYS];
    __shared__ float mred[ACL_THREADS / 64];
    const int tid = threadIdx.x, s = tid & 7, g = tid >> 3;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H, L = p.L;
    int n = L;
    if (KEYPAD) {
        n = p.keylen[b];
        n = n < 1 ? 1 : (n > L ? L : n);
    }
    const size_t row0 = (size_t)b * L;
    const int col = h * 64 + 8 * s;
    float q[8];
    load8((const T*)p.q + row0 * p.ld_qkv + col, q);
    float sc[ACL_PASSES];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < ACL_PASSES; ++t) {
        const int j = t * ACL_KEYS + g;
        sc[t] = -INFINITY;
        if (j < n) {
            float k[8];
            load8((const T*)p.k + (row0 + j) * p.ld_qkv + col, k);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) d = fmaf(q[e], k[e], d);
            sc[t] = sum8(d) * p.scale;
            m = fmaxf(m, sc[t]);
        }
    }
    m = wave_max(m);
    if ((tid & 63) == 0) mred[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));          // key 0 is always valid: m is finite
    float o[8], l = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int t = 0; t < ACL_PASSES; ++t) {
        const int j = t * ACL_KEYS + g;
        if (j < n) {
            float v[8];
            load8((const T*)p.v + (row0 + j) * p.ld_qkv + col, v);
            const float P = __expf(sc[t] - m);
            l += P;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = fmaf(P, v[e], o[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[g][8 * s + e] = o[e];
    if (s == 0) lred[g] = l;
    __syncthreads();
    if (tid < 8) {
        float acc[8], lsum = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int r = 0; r < ACL_KEYS; ++r) {
            lsum += lred[r];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += red[r][8 * tid + e];
        }
        const float inv = 1.0f / lsum;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= inv;
        store8((T*)p.out + (size_t)b * p.ldo + h * 64 + 8 * tid, acc);
        if (tid == 0 && p.lse) p.lse[(size_t)b * p.H + h] = m + __logf(lsum);
    }
}

// d[b, c] = keep_scale(b·ntok·64 + c) · gelu(t[b, c]): the CLS branch of mona_spatial's forward (csrc/mona.hip), same operands, same order
template <typename T>
__global__ __launch_bounds__(256) void mona_cls_fwd_kernel(int B, int ntok, const T* __restrict__ t, long ldt, T* __restrict__ d, float p_drop, uint64_t seed,
                                                           const uint8_t* __restrict__ keep_mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * 64) return;
    const int b = i >> 6, c = i & 63;
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const uint32_t thresh = p_drop > 0.f ? (uint32_t)fminf(p_drop * 4294967296.0f, 4294967295.0f) : 0u;
    const size_t idx = (size_t)b * ntok * 64 + c;
    float ks = 1.0f;
    if (keep_mask) ks = keep_mask[idx] ? inv_keep : 0.f;
    else if (p_drop > 0.f) ks = dropout_keep(seed, (uint32_t)idx, thresh) ? inv_keep : 0.f;
    const float z = to_f32(t[(size_t)b * ldt + c]);
    d[i] = from_f32<T>(gelu_erf(z) * ks);
}

// dst[r, c] = the fp32 value of element (r·stride, c) of a three-byte tensor: float bits = (hi bits << 16) + (lo << 8)
__global__ __launch_bounds__(256) void rows3_kernel(int rows, int D, long stride, const uint16_t* __restrict__ hi, long ldhi, long hi_kb_rows, const int8_t* __restrict__ lo,
                                                    long ldlo, float* __restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * D) return;
    const long r = i / D, row = r * stride;
    const int c = (int)(i - r * D);
    const uint32_t hb = hi_kb_rows ? hi[((long)(c >> 5) * hi_kb_rows + row) * 32 + (c & 31)] : hi[row * ldhi + c];
    const int32_t lb = lo[row * ldlo + c];
    dst[i] = __builtin_bit_cast(float, (hb << 16) + ((uint32_t)lb << 8));
}

// dt[b, c] = dd[b, c] · keep_scale(b·ntok·64 + c) · gelu'(t[b·ntok, c]): the CLS branch of mona_spatial's backward (csrc/mona.hip), same operands, same order
template <typename T>
__global__ __launch_bounds__(256) void mona_cls_bwd_kernel(int B, int ntok, const T* __restrict__ dd, const T* __restrict__ t, long ldt, T* __restrict__ dt,
                                                           float p_drop, uint64_t seed, const uint8_t* __restrict__ keep_mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * 64) return;
    const int b = i >> 6, c = i & 63;
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const uint32_t thresh = p_drop > 0.f ? (uint32_t)fminf(p_drop * 4294967296.0f, 4294967295.0f) : 0u;
    const size_t idx = (size_t)b * ntok * 64 + c;
    float ks = 1.0f;
    if (keep_mask) ks = keep_mask[idx] ? inv_keep : 0.f;
    else if (p_drop > 0.f) ks = dropout_keep(seed, (uint32_t)idx, thresh) ? inv_keep : 0.f;
    const float z = to_f32(t[(size_t)b * ldt + c]);
    dt[i] = from_f32<T>(to_f32(dd[i]) * ks * dgelu_erf(z));
}

__global__ __launch_bounds__(256) void copy_rows_kernel(int rows, int units, const uint4* __restrict__ src, long src_stride_units, uint4* __restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * units) return;
    const long r = i / units, u = i - r * units;
    dst[i] = src[r * src_stride_units + u];
}

}  // namespace

int uia_attn_bwd_cls_launch(hipStream_t stream, int dtype, const UiaAttnParams& p, bool compact) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_attn_bwd_cls: bad dtype %d", dtype);
    UIA_CHECK_ARG(p.B > 0 && p.H > 0 && p.L > 0 && p.L <= 288, "uia_attn_bwd_cls: B=%d H=%d L=%d outside the supported range (L <= 288)", p.B, p.H, p.L);
    UIA_CHECK_ARG(p.dh == 64, "uia_attn_bwd_cls: head dim %d, only 64 is supported", p.dh);
    UIA_CHECK_ARG(p.mask_kind == UIA_MASK_NONE && !p.keylen && !p.cu_seqlens, "uia_attn_bwd_cls: no mask, no key lengths, no packed sequences (mask kind %d)", p.mask_kind);
    UIA_CHECK_ARG(p.scale > 0.f && p.scale < 3.0e38f, "uia_attn_bwd_cls: scale must be positive and finite, got %g", (double)p.scale);
    UIA_CHECK_ARG(p.q && p.k && p.v && p.out && p.dout && p.lse && p.dq && p.dk && p.dv, "uia_attn_bwd_cls: null tensor");
    UIA_CHECK_ARG(!compact || p.out_kb_rows == 0, "uia_attn_bwd_cls_rows: out holds one row-major row per sequence, not a K-blocked tensor");
    UIA_CHECK_ARG((p.out_kb_rows == 0 && p.dqkv_kb_rows == 0) ||
                  (dtype == UIA_BF16 && (p.out_kb_rows == 0 || p.out_kb_rows >= (int64_t)p.B * p.L) && (p.dqkv_kb_rows == 0 || p.dqkv_kb_rows >= (int64_t)p.B * p.L)),
                  "uia_attn_bwd_cls: K-blocked out / dq, dk, dv need bf16 and at least B*L rows");
    const int esz = dtype == UIA_BF16 ? 2 : 4;
    const int64_t width = (int64_t)p.H * 64;
    UIA_CHECK_ARG(p.ld_qkv >= width && p.lddo >= width && (p.out_kb_rows || p.ldo >= width) && (p.dqkv_kb_rows || p.ld_dqkv >= width), "uia_attn_bwd_cls: leading dimension below H*64");
    UIA_CHECK_ARG((p.ld_qkv * esz) % 16 == 0 && (p.ldo * esz) % 16 == 0 && (p.lddo * esz) % 16 == 0 && (p.ld_dqkv * esz) % 16 == 0,
                  "uia_attn_bwd_cls: leading dimensions must keep 16-byte rows");
    UIA_CHECK_ARG(((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.out | (uintptr_t)p.dout | (uintptr_t)p.dq | (uintptr_t)p.dk | (uintptr_t)p.dv) % 16 == 0,
                  "uia_attn_bwd_cls: alignment");
    const dim3 grid(p.B * p.H), block(ACL_THREADS);
    if (dtype == UIA_BF16) hipLaunchKernelGGL((attn_bwd_cls_kernel<bf16_t, true>), grid, block, 0, stream, p, (int)compact);
    else hipLaunchKernelGGL((attn_bwd_cls_kernel<float, false>), grid, block, 0, stream, p, (int)compact);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_attn_fwd_cls_launch(hipStream_t stream, int dtype, const UiaAttnParams& p) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_attn_fwd_cls: bad dtype %d", dtype);
    UIA_CHECK_ARG(p.B > 0 && p.H > 0 && p.L > 0 && p.L <= ACL_MAX_L, "uia_attn_fwd_cls: B=%d H=%d L=%d outside the supported range (L <= 288)", p.B, p.H, p.L);
    UIA_CHECK_ARG(p.dh == 64, "uia_attn_fwd_cls: head dim %d, only 64 is supported", p.dh);
    UIA_CHECK_ARG(!p.cu_seqlens && ((p.mask_kind == UIA_MASK_NONE && !p.keylen) || (p.mask_kind == UIA_MASK_KEYPAD && p.keylen)),
                  "uia_attn_fwd_cls: mask kind %d: none (without key lengths) or key padding (with them), no packed sequences", p.mask_kind);
    UIA_CHECK_ARG(p.scale > 0.f && p.scale < 3.0e38f, "uia_attn_fwd_cls: scale must be positive and finite, got %g", (double)p.scale);
    UIA_CHECK_ARG(p.q && p.k && p.v && p.out, "uia_attn_fwd_cls: null tensor");
    UIA_CHECK_ARG(p.out_kb_rows == 0, "uia_attn_fwd_cls: out holds one row-major row per sequence, not a K-blocked tensor");
    const int esz = dtype == UIA_BF16 ? 2 : 4;
    const int64_t width = (int64_t)p.H * 64;
    UIA_CHECK_ARG(p.ld_qkv >= width && p.ldo >= width, "uia_attn_fwd_cls: leading dimension below H*64");
    UIA_CHECK_ARG((p.ld_qkv * esz) % 16 == 0 && (p.ldo * esz) % 16 == 0, "uia_attn_fwd_cls: leading dimensions must keep 16-byte rows");
    UIA_CHECK_ARG(((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.out) % 16 == 0 && (uintptr_t)p.lse % 4 == 0 && (uintptr_t)p.keylen % 4 == 0,
                  "uia_attn_fwd_cls: alignment");
    const dim3 grid(p.B * p.H), block(ACL_THREADS);
    const bool kp = p.mask_kind == UIA_MASK_KEYPAD;
    if (dtype == UIA_BF16) {
        if (kp) hipLaunchKernelGGL((attn_fwd_cls_kernel<bf16_t, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_fwd_cls_kernel<bf16_t, false>), grid, block, 0, stream, p);
    } else {
        if (kp) hipLaunchKernelGGL((attn_fwd_cls_kernel<float, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((attn_fwd_cls_kernel<float, false>), grid, block, 0, stream, p);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_mona_cls_fwd_launch(hipStream_t stream, int dtype, int B, int ntok, const void* t, long ldt, void* d, float p_drop, uint64_t seed, const uint8_t* keep_mask) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_mona_cls_fwd: bad dtype %d", dtype);
    UIA_CHECK_ARG(B > 0 && ntok > 0 && (size_t)B * ntok * 64 <= 0xFFFFFFFFull, "uia_mona_cls_fwd: B=%d images of %d tokens outside the 32-bit mask index", B, ntok);
    UIA_CHECK_ARG(t && d && ldt >= 64, "uia_mona_cls_fwd: null tensor or row stride below 64");
    UIA_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "uia_mona_cls_fwd: p_drop=%f outside [0, 1)", (double)p_drop);
    const dim3 grid((B * 64 + 255) / 256), block(256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(mona_cls_fwd_kernel<bf16_t>, grid, block, 0, stream, B, ntok, (const bf16_t*)t, ldt, (bf16_t*)d, p_drop, seed, keep_mask);
    else hipLaunchKernelGGL(mona_cls_fwd_kernel<float>, grid, block, 0, stream, B, ntok, (const float*)t, ldt, (float*)d, p_drop, seed, keep_mask);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_rows3_to_f32_launch(hipStream_t stream, int rows, int D, long stride_rows, const void* hi, long ldhi, long hi_kb_rows, const int8_t* lo, long ldlo, float* dst) {
    UIA_CHECK_ARG(rows > 0 && D > 0 && stride_rows > 0 && (long)rows * D <= 0x7FFFFFFFL, "uia_rows3_to_f32: %d rows of %d elements, %ld apart", rows, D, stride_rows);
    UIA_CHECK_ARG(hi && lo && dst && ldlo >= D, "uia_rows3_to_f32: null plane, or low-byte rows closer than D");
    UIA_CHECK_ARG(hi_kb_rows ? (D % 32 == 0 && hi_kb_rows > (long)(rows - 1) * stride_rows) : ldhi >= D,
                  "uia_rows3_to_f32: hi plane: row-major rows closer than D, or a K-blocked plane of %ld rows that does not hold row %ld in whole 32-element blocks", hi_kb_rows,
                  (long)(rows - 1) * stride_rows);
    const long total = (long)rows * D;
    hipLaunchKernelGGL(rows3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, rows, D, stride_rows, (const uint16_t*)hi, ldhi, hi_kb_rows, lo, ldlo, dst);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_mona_cls_bwd_launch(hipStream_t stream, int dtype, int B, int ntok, const void* dd, const void* t, long ldt, void* dt, float p_drop, uint64_t seed,
                            const uint8_t* keep_mask) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_mona_cls_bwd: bad dtype %d", dtype);
    UIA_CHECK_ARG(B > 0 && ntok > 0 && (size_t)B * ntok * 64 <= 0xFFFFFFFFull, "uia_mona_cls_bwd: B=%d images of %d tokens outside the 32-bit mask index", B, ntok);
    UIA_CHECK_ARG(dd && t && dt && ldt >= 64, "uia_mona_cls_bwd: null tensor or row stride below 64");
    UIA_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "uia_mona_cls_bwd: p_drop=%f outside [0, 1)", (double)p_drop);
    const dim3 grid((B * 64 + 255) / 256), block(256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(mona_cls_bwd_kernel<bf16_t>, grid, block, 0, stream, B, ntok, (const bf16_t*)dd, (const bf16_t*)t, ldt, (bf16_t*)dt, p_drop, seed, keep_mask);
    else hipLaunchKernelGGL(mona_cls_bwd_kernel<float>, grid, block, 0, stream, B, ntok, (const float*)dd, (const float*)t, ldt, (float*)dt, p_drop, seed, keep_mask);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_copy_rows_launch(hipStream_t stream, int rows, long row_bytes, const void* src, long src_stride_bytes, void* dst) {
    UIA_CHECK_ARG(rows > 0 && row_bytes > 0 && row_bytes % 16 == 0 && src_stride_bytes % 16 == 0 && src_stride_bytes >= row_bytes && row_bytes / 16 <= 0x7FFFFFFF,
                  "uia_copy_rows: %d rows of %ld bytes, %ld apart: rows and their stride must be whole 16-byte units", rows, row_bytes, src_stride_bytes);
    UIA_CHECK_ARG(src && dst && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "uia_copy_rows: null or misaligned tensor");
    const int units = (int)(row_bytes / 16);
    const long total = (long)rows * units;
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, rows, units, (const uint4*)src, src_stride_bytes / 16, (uint4*)dst);
    UIA_CHECK_LAUNCH();
    return 0;
}
