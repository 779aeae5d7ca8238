// cls_grad.hip — the backward of the last image block and its adapter when the gradient is CLS-sparse.
//
// The contrastive head reads token 0 of every image only, so the gradient that enters the last adapter and the MLP half of the last block is
// non-zero in one row of every 1 + h·w.  Those stages work row by row and run on the B CLS rows through the ordinary launches; what is
// left for this file is the three places where the sparse rows meet a dense tensor:
//   attn_bwd_cls_kernel   attention backward with ONE non-zero query row per head; writes the whole dense dq / dk / dv
//   mona_cls_bwd_kernel   the adapter's dropout · GELU' on the CLS token (it bypasses the spatial operator), mask index of the DENSE tensor
//   copy_rows_kernel      rows of any 16-byte-granular type out of a strided tensor (row b·N of a saved activation)
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
__global__ __launch_bounds__(ACL_THREADS) void attn_bwd_cls_kernel(const UiaAttnParams p) {
    __shared__ float red[ACL_KEYS][64];
    const int tid = threadIdx.x, s = tid & 7, g = tid >> 3;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H, L = p.L;
    const size_t row0 = (size_t)b * L;
    const int col = h * 64 + 8 * s;
    float q[8], o[8], dO[8];
    load8((const T*)p.q + row0 * p.ld_qkv + col, q);
    load8((const T*)p.dout + (size_t)b * p.lddo + col, dO);
    if (KB && p.out_kb_rows) load8((const T*)p.out + ((size_t)(col >> 5) * (size_t)p.out_kb_rows + row0) * 32 + (col & 31), o);
    else load8((const T*)p.out + row0 * p.ldo + col, o);
    const float lse = p.lse[((size_t)b * p.H + h) * L];
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

int uia_attn_bwd_cls_launch(hipStream_t stream, int dtype, const UiaAttnParams& p) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_attn_bwd_cls: bad dtype %d", dtype);
    UIA_CHECK_ARG(p.B > 0 && p.H > 0 && p.L > 0 && p.L <= 288, "uia_attn_bwd_cls: B=%d H=%d L=%d outside the supported range (L <= 288)", p.B, p.H, p.L);
    UIA_CHECK_ARG(p.dh == 64, "uia_attn_bwd_cls: head dim %d, only 64 is supported", p.dh);
    UIA_CHECK_ARG(p.mask_kind == UIA_MASK_NONE && !p.keylen && !p.cu_seqlens, "uia_attn_bwd_cls: no mask, no key lengths, no packed sequences (mask kind %d)", p.mask_kind);
    UIA_CHECK_ARG(p.scale > 0.f && p.scale < 3.0e38f, "uia_attn_bwd_cls: scale must be positive and finite, got %g", (double)p.scale);
    UIA_CHECK_ARG(p.q && p.k && p.v && p.out && p.dout && p.lse && p.dq && p.dk && p.dv, "uia_attn_bwd_cls: null tensor");
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
    if (dtype == UIA_BF16) hipLaunchKernelGGL((attn_bwd_cls_kernel<bf16_t, true>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((attn_bwd_cls_kernel<float, false>), grid, block, 0, stream, p);
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
