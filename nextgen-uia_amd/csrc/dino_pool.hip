// dino_pool.hip — mean over a run of token rows of their LayerNorm: out[b, :] = mean_{l in [row0, row0+n)} LN(x[b, l, :]).
//
// Replaces: the patch-token half of the DINOv2 classification head's features (the reference's src/third_party/dino/dinov2.py:33-100:
//           torch.mean(norm(x)[:, 1:], dim=1) of the last block), without writing the normalised [B·L, D] tensor first.
//
// mean_l (x_l − μ_l)·r_l·γ + β  =  γ ⊙ mean_l (x_l − μ_l)·r_l + β:  the affine part is applied once per column at the end.
// Two launches with a fixed reduction order (no atomics, bit-identical from run to run):
//   1. grid (B, POOL_SLICES): each workgroup takes a contiguous slice of the rows; each wave normalises its rows (two-pass statistics
//      held in registers, as layernorm.hip) and sums them per column; the four waves' sums are added in wave order through LDS.
//   2. grid B: the slices are added in slice order, scaled by γ/n and shifted by β.
// fp32 rows with stride ldx (elements) between tokens and L·ldx between images; D ≤ 1024, D % 4 == 0.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int POOL_V = 4;      // float4 per lane -> D <= 1024

__global__ __launch_bounds__(256) void ln_mean_partial_kernel(int L, int row0, int n, int D, long ldx, const float* __restrict__ x, float eps,
                                                              float* __restrict__ ws) {
    __shared__ f32x4 part[4][64 * POOL_V];
    const int b = blockIdx.x, sl = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per = (n + UIA_POOL_SLICES - 1) / UIA_POOL_SLICES;
    const int r_begin = sl * per, r_end = r_begin + per < n ? r_begin + per : n;
    const int nv = D >> 2;
    f32x4 acc[POOL_V];
#pragma unroll
    for (int k = 0; k < POOL_V; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = r_begin + wave; r < r_end; r += 4) {
        const float* xr = x + ((size_t)b * L + row0 + r) * ldx;
        f32x4 v[POOL_V];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < POOL_V; ++k) {
            const int c = lane + 64 * k;
            v[k] = c < nv ? load4(xr + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
            s += v[k][0] + v[k][1] + v[k][2] + v[k][3];
        }
        const float mean = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < POOL_V; ++k) {
            const int c = lane + 64 * k;
            if (c < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[k][e] - mean; q = fmaf(d, d, q); }
            }
        }
        const float rstd = rsqrtf(wave_sum(q) / D + eps);
#pragma unroll
        for (int k = 0; k < POOL_V; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[k][e] += (v[k][e] - mean) * rstd;
    }
#pragma unroll
    for (int k = 0; k < POOL_V; ++k) part[wave][lane + 64 * k] = acc[k];
    __syncthreads();
    if (wave == 0) {
        float* dst = ws + ((size_t)b * UIA_POOL_SLICES + sl) * D;
#pragma unroll
        for (int k = 0; k < POOL_V; ++k) {
            const int c = lane + 64 * k;
            if (c < nv) {
                f32x4 t = part[0][c];
#pragma unroll
                for (int w = 1; w < 4; ++w) {
                    const f32x4 u = part[w][c];
                    t = f32x4{t[0] + u[0], t[1] + u[1], t[2] + u[2], t[3] + u[3]};
                }
                store4(dst + 4 * c, t);
            }
        }
    }
}

__global__ __launch_bounds__(256) void ln_mean_final_kernel(int n, int D, const float* __restrict__ ws, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ out, long ldo) {
    const int b = blockIdx.x;
    const float inv = 1.0f / n;
    for (int c = threadIdx.x; c < (D >> 2); c += 256) {
        f32x4 t = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < UIA_POOL_SLICES; ++sl) {
            const f32x4 u = load4(ws + ((size_t)b * UIA_POOL_SLICES + sl) * D + 4 * c);
            t = f32x4{t[0] + u[0], t[1] + u[1], t[2] + u[2], t[3] + u[3]};
        }
        const f32x4 g = load4(gamma + 4 * c), be = load4(beta + 4 * c);
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = fmaf(t[e] * inv, g[e], be[e]);
        store4(out + (size_t)b * ldo + 4 * c, y);
    }
}

}  // namespace

int uia_ln_mean_rows_launch(hipStream_t stream, int B, int L, int row0, int n, int D, long ldx, const float* x, const float* gamma, const float* beta,
                            float eps, float* ws, float* out, long ldo) {
    UIA_CHECK_ARG(B > 0 && L > 0 && n > 0 && row0 >= 0 && row0 + n <= L, "uia_ln_mean_rows: rows [%d, %d) outside the %d tokens of an image", row0, row0 + n, L);
    UIA_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 1024, "uia_ln_mean_rows: D=%d must be a multiple of 4 and <= 1024", D);
    UIA_CHECK_ARG(ldx >= D && ldx % 4 == 0 && ldo >= D && ldo % 4 == 0, "uia_ln_mean_rows: leading dimensions must be >= D and multiples of 4");
    UIA_CHECK_ARG(x && gamma && beta && ws && out, "uia_ln_mean_rows: null tensor");
    UIA_CHECK_ARG(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)ws | (uintptr_t)out) % 16 == 0, "uia_ln_mean_rows: pointers must be 16-byte aligned");
    UIA_CHECK_ARG(eps >= 0.f, "uia_ln_mean_rows: eps must be >= 0");
    hipLaunchKernelGGL(ln_mean_partial_kernel, dim3(B, UIA_POOL_SLICES), dim3(256), 0, stream, L, row0, n, D, ldx, x, eps, ws);
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(ln_mean_final_kernel, dim3(B), dim3(256), 0, stream, n, D, ws, gamma, beta, out, ldo);
    UIA_CHECK_LAUNCH();
    return 0;
}
