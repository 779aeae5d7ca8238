// unet_bn.hip — BatchNorm2d + ReLU of the DINOv2 UNet decoder on NHWC rows [M = B·H·W, C], plain column sums (the convs' bias
// gradients), and BatchNorm2d + LeakyReLU + Dropout of the baseline UNet's ConvBlock (the reference's src/third_party/unet.py:10-18) on the
// same statistics kernels.
//
// Replaces: nn.BatchNorm2d(eps 1e-5, momentum 0.1) + nn.ReLU of UNetDecoderUpBlock (the reference's src/third_party/dino/dinov2.py:130-152)
//           in training and eval mode, forward and backward.
//
// Every reduction runs in two launches with a fixed order (no atomics, bit-identical from run to run):
//   1. grid S (at most UIA_BN_SLICES): workgroup s takes a contiguous run of rows; its threads own (channel, row lane) pairs, each sums
//      its rows in order and the row lanes are added in lane order through LDS: two floats per (slice, channel).
//   2. one thread per channel adds the slices in slice order.
// The batch statistics are summed shifted by the slice's first row (Σ(y − K), Σ(y − K)²) and combined with Chan's formula, so a large
// mean does not cancel the variance.  Nothing is read back on the host: the running buffers and num_batches_tracked are updated here.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

enum { RED_STATS = 0, RED_BWD = 1, RED_SUM = 2 };

// ws[(s·C + c)·3 + {0,1,2}]: RED_STATS {Σ(y−K), Σ(y−K)², K}; RED_BWD {Σdz, Σdz·x̂, 0}; RED_SUM {Σy, 0, 0}
template <typename T, int MODE>
__global__ __launch_bounds__(256) void reduce_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ ws) {
    __shared__ float red[2][256];
    const int S = gridDim.x, s = blockIdx.x, tid = threadIdx.x;
    const long per = (M + S - 1) / S;
    const long rb = (long)s * per, re = rb + per < M ? rb + per : M;
    const int Cb = C < 256 ? C : 256, RP = 256 / Cb;
    for (int cbase = 0; cbase < C; cbase += Cb) {
        const int c = cbase + tid % Cb, rl = tid / Cb;
        const bool act = rl < RP && c < C;
        float a = 0.f, q = 0.f, K = 0.f;
        if (act && rb < re) {
            if (MODE == RED_STATS) K = to_f32(y[rb * C + c]);
            float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
            if (MODE == RED_BWD) { sc = scale[c]; sh = shift[c]; mu = mean[c]; is = invstd[c]; }
            for (long r = rb + rl; r < re; r += RP) {
                const float v = to_f32(y[r * C + c]);
                if (MODE == RED_STATS) {
                    const float d = v - K;
                    a += d;
                    q = fmaf(d, d, q);
                } else if (MODE == RED_BWD) {
                    const float dz = fmaf(v, sc, sh) > 0.f ? to_f32(dout[r * C + c]) : 0.f;
                    a += dz;
                    q = fmaf(dz, (v - mu) * is, q);
                } else {
                    a += v;
                }
            }
        }
        red[0][tid] = a;
        red[1][tid] = q;
        __syncthreads();
        if (rl == 0 && c < C) {
            for (int k = 1; k < RP; ++k) {
                a += red[0][tid + k * Cb];
                q += red[1][tid + k * Cb];
            }
            float* o = ws + ((size_t)s * C + c) * 3;
            o[0] = a;
            o[1] = q;
            o[2] = K;
        }
        __syncthreads();
    }
}

// train-mode statistics: mean, 1/std, the affine scale / shift of the apply, running buffers
__global__ __launch_bounds__(256) void bn_finalize_kernel(long M, int C, int S, const float* __restrict__ ws, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, float momentum, float* __restrict__ mean,
                                                          float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift,
                                                          float* __restrict__ run_mean, float* __restrict__ run_var, int64_t* __restrict__ nbt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c == 0 && nbt) nbt[0] += 1;
    if (c >= C) return;
    const long per = (M + S - 1) / S;
    double n = 0.0, mu = 0.0, m2 = 0.0;      // Chan's parallel combination, slice by slice (fp64 only for these few per-channel scalars)
    for (int s = 0; s < S; ++s) {
        const long rb = (long)s * per, re = rb + per < M ? rb + per : M;
        if (re <= rb) continue;
        const double ns = (double)(re - rb);
        const float* o = ws + ((size_t)s * C + c) * 3;
        const double ms = (double)o[2] + (double)o[0] / ns;
        const double m2s = (double)o[1] - (double)o[0] * (double)o[0] / ns;
        const double nn = n + ns, d = ms - mu;
        mu += d * ns / nn;
        m2 += m2s + d * d * n * ns / nn;
        n = nn;
    }
    const double var = m2 > 0.0 ? m2 / n : 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    mean[c] = (float)mu;
    invstd[c] = is;
    const float g = gamma[c] * is;
    scale[c] = g;
    shift[c] = beta[c] - (float)mu * g;
    if (run_mean) {
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mu;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(n > 1.0 ? m2 / (n - 1.0) : var);
    }
}

__global__ __launch_bounds__(256) void bn_eval_coeff_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ run_mean, const float* __restrict__ run_var, float eps,
                                                            float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float g = gamma[c] / sqrtf(run_var[c] + eps);
    scale[c] = g;
    shift[c] = beta[c] - run_mean[c] * g;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(long n, int C, const T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int relu, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = fmaf(to_f32(y[i]), scale[c], shift[c]);
    if (relu) v = v > 0.f ? v : 0.f;
    out[i] = from_f32<T>(v);
}

// column sums (RED_SUM) or the two BN backward sums (RED_BWD), slices added in order
__global__ __launch_bounds__(256) void col_finalize_kernel(int C, int S, const float* __restrict__ ws, float* __restrict__ o0, float* __restrict__ o1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, q = 0.f;
    for (int s = 0; s < S; ++s) {
        a += ws[((size_t)s * C + c) * 3];
        q += ws[((size_t)s * C + c) * 3 + 1];
    }
    o0[c] = a;
    if (o1) o1[c] = q;
}

// dy = γ·r·(dz − Σdz/M − x̂·Σ(dz·x̂)/M), dz = dout·[y·scale + shift > 0]
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ dbeta, const float* __restrict__ dgamma,
                                                           T* __restrict__ dy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int c = (int)(i % C);
    const float v = to_f32(y[i]);
    const float dz = fmaf(v, scale[c], shift[c]) > 0.f ? to_f32(dout[i]) : 0.f;
    const float is = invstd[c], xh = (v - mean[c]) * is, inv = 1.0f / (float)M;
    dy[i] = from_f32<T>(gamma[c] * is * (dz - dbeta[c] * inv - xh * dgamma[c] * inv));
}

// ---------------------------------------------------------------- BatchNorm + LeakyReLU + Dropout (the baseline UNet's ConvBlock)
// keep·1/(1−p) of element i: the explicit mask, else the draw of uia_dropout (one dropout_keep8 per eight consecutive elements)
struct Drop {
    const uint8_t* mask;
    uint64_t seed;
    uint32_t thresh16;
    float inv_keep;
    int on;
};
__device__ __forceinline__ float drop_factor(const Drop& d, long i) {
    if (!d.on) return 1.f;
    const bool keep = d.mask ? d.mask[i] != 0 : ((dropout_keep8(d.seed, (uint32_t)(i >> 3), d.thresh16) >> (i & 7)) & 1u) != 0;
    return keep ? d.inv_keep : 0.f;
}
// the factors of the eight consecutive elements starting at i0 (a multiple of 8): one draw of the generator, or eight mask bytes in one load
__device__ __forceinline__ void drop_factors8(const Drop& d, long i0, float (&k)[8]) {
    if (d.mask) {
        const uint64_t m = *(const uint64_t*)(d.mask + i0);
#pragma unroll
        for (int e = 0; e < 8; ++e) k[e] = (m >> (8 * e)) & 0xFFu ? d.inv_keep : 0.f;
    } else {
        const uint32_t m = dropout_keep8(d.seed, (uint32_t)(i0 >> 3), d.thresh16);
#pragma unroll
        for (int e = 0; e < 8; ++e) k[e] = (m >> e) & 1u ? d.inv_keep : 0.f;
    }
}
// the eight-element kernels serve both kinds of mask under the same conditions, so a generated mask and the same mask passed explicitly give
// the same bits: dropout on, a multiple of 8 elements, 16-byte-aligned tensors (8-byte-aligned mask)
bool drop8_ok(const Drop& d, long n, const void* a, const void* b, const void* c) {
    return d.on && n % 8 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0) && (((uintptr_t)d.mask & 7) == 0);
}
// dz = dout·keep/(1−p)·leaky'(z); z == 0 takes the slope, as PyTorch's leaky_relu backward
__device__ __forceinline__ float act_dz(float z, float dout, float slope, const Drop& d, long i) {
    float g = dout;
    if (d.on) g *= drop_factor(d, i);
    return z > 0.f ? g : g * slope;
}

// one element of the forward before dropout, and of the backward after dz: shared by the one- and the eight-element kernels
__device__ __forceinline__ float act_fwd_elem(float y, float sc, float sh, float slope) {
    const float v = fmaf(y, sc, sh);
    return v > 0.f ? v : (slope == 0.f ? 0.f : slope * v);
}
__device__ __forceinline__ float bn_bwd_elem(float v, float dz, float mu, float is, float gamma, float dbeta, float dgamma, float inv) {
    const float xh = (v - mu) * is;
    return gamma * is * (dz - dbeta * inv - xh * dgamma * inv);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_act_apply_kernel(long n, int C, const T* __restrict__ y, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float slope, Drop d, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = act_fwd_elem(to_f32(y[i]), scale[c], shift[c], slope);
    if (d.on) v *= drop_factor(d, i);
    out[i] = from_f32<T>(v);
}

// the same with dropout on: eight consecutive elements per thread, so one draw of the generator serves the eight it covers
template <typename T>
__global__ __launch_bounds__(256) void bn_act_apply8_kernel(long n, int C, const T* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float slope, Drop d, T* __restrict__ out) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= n) return;
    float v[8], k[8];
    load8(y + i0, v);
    drop_factors8(d, i0, k);
    int c = (int)(i0 % C);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = act_fwd_elem(v[e], scale[c], shift[c], slope) * k[e];
        if (++c == C) c = 0;
    }
    store8(out + i0, v);
}

// reduce_kernel<RED_BWD> with the activation's dz
template <typename T>
__global__ __launch_bounds__(256) void reduce_act_bwd_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd, float slope, Drop d,
                                                             float* __restrict__ ws) {
    __shared__ float red[2][256];
    const int S = gridDim.x, s = blockIdx.x, tid = threadIdx.x;
    const long per = (M + S - 1) / S;
    const long rb = (long)s * per, re = rb + per < M ? rb + per : M;
    const int Cb = C < 256 ? C : 256, RP = 256 / Cb;
    for (int cbase = 0; cbase < C; cbase += Cb) {
        const int c = cbase + tid % Cb, rl = tid / Cb;
        const bool act = rl < RP && c < C;
        float a = 0.f, q = 0.f;
        if (act && rb < re) {
            const float sc = scale[c], sh = shift[c], mu = mean[c], is = invstd[c];
            for (long r = rb + rl; r < re; r += RP) {
                const float v = to_f32(y[r * C + c]);
                const float dz = act_dz(fmaf(v, sc, sh), to_f32(dout[r * C + c]), slope, d, r * C + c);
                a += dz;
                q = fmaf(dz, (v - mu) * is, q);
            }
        }
        red[0][tid] = a;
        red[1][tid] = q;
        __syncthreads();
        if (rl == 0 && c < C) {
            for (int k = 1; k < RP; ++k) {
                a += red[0][tid + k * Cb];
                q += red[1][tid + k * Cb];
            }
            float* o = ws + ((size_t)s * C + c) * 3;
            o[0] = a;
            o[1] = q;
            o[2] = 0.f;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ dbeta, const float* __restrict__ dgamma,
                                                               float slope, Drop d, T* __restrict__ dy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int c = (int)(i % C);
    const float v = to_f32(y[i]);
    const float dz = act_dz(fmaf(v, scale[c], shift[c]), to_f32(dout[i]), slope, d, i);
    dy[i] = from_f32<T>(bn_bwd_elem(v, dz, mean[c], invstd[c], gamma[c], dbeta[c], dgamma[c], 1.0f / (float)M));
}

// the same with dropout on, eight consecutive elements per thread (see bn_act_apply8_kernel)
template <typename T>
__global__ __launch_bounds__(256) void bn_act_bwd_apply8_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ dbeta, const float* __restrict__ dgamma,
                                                                float slope, Drop d, T* __restrict__ dy) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= M * C) return;
    float v[8], g[8], k[8];
    load8(y + i0, v);
    load8(dout + i0, g);
    drop_factors8(d, i0, k);
    const float inv = 1.0f / (float)M;
    int c = (int)(i0 % C);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gk = g[e] * k[e];
        const float dz = fmaf(v[e], scale[c], shift[c]) > 0.f ? gk : gk * slope;
        v[e] = bn_bwd_elem(v[e], dz, mean[c], invstd[c], gamma[c], dbeta[c], dgamma[c], inv);
        if (++c == C) c = 0;
    }
    store8(dy + i0, v);
}

int slices_for(long M) { long s = (M + 255) / 256; return (int)(s < UIA_BN_SLICES ? s : UIA_BN_SLICES); }

}  // namespace

#define BN_ARGS_OK(fn)                                                                                                      \
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, fn ": dtype must be UIA_F32 or UIA_BF16");                       \
    UIA_CHECK_ARG(M > 0 && C > 0 && C <= 65536 && M < (1l << 40), fn ": M=%ld C=%d out of range", (long)M, C)

int uia_colsum_ordered_launch(hipStream_t stream, int dtype, long M, int C, const void* y, float* ws, float* out) {
    BN_ARGS_OK("uia_colsum_ordered");
    UIA_CHECK_ARG(y && ws && out, "uia_colsum_ordered: null tensor");
    const int S = slices_for(M);
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL((reduce_kernel<bf16_t, RED_SUM>), dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
    else
        hipLaunchKernelGGL((reduce_kernel<float, RED_SUM>), dim3(S), dim3(256), 0, stream, M, C, (const float*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, S, ws, out, nullptr);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const float* gamma, const float* beta,
                      float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean, float* invstd,
                      float* scale, float* shift, int relu, void* out) {
    BN_ARGS_OK("uia_bn_fwd");
    UIA_CHECK_ARG(y && gamma && beta && scale && shift && out, "uia_bn_fwd: null tensor");
    UIA_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "uia_bn_fwd: eps must be > 0 and momentum in [0, 1]");
    if (training) {
        UIA_CHECK_ARG(ws && mean && invstd, "uia_bn_fwd: training needs ws, mean and invstd");
        UIA_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "uia_bn_fwd: running mean and variance come together");
        const int S = slices_for(M);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL((reduce_kernel<bf16_t, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        else
            hipLaunchKernelGGL((reduce_kernel<float, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const float*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        UIA_CHECK_LAUNCH();
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, M, C, S, ws, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                           run_mean, run_var, nbt);
    } else {
        UIA_CHECK_ARG(run_mean && run_var, "uia_bn_fwd: eval mode needs the running buffers");
        hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, gamma, beta, run_mean, run_var, eps, scale, shift);
    }
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const bf16_t*)y, scale, shift, relu, (bf16_t*)out);
    else
        hipLaunchKernelGGL(bn_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const float*)y, scale, shift, relu, (float*)out);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_relu_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                           const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy) {
    BN_ARGS_OK("uia_bn_relu_bwd");
    UIA_CHECK_ARG(y && dout && scale && shift && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_relu_bwd: null tensor");
    const int S = slices_for(M);
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL((reduce_kernel<bf16_t, RED_BWD>), dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)dout, scale, shift, mean, invstd, ws);
    else
        hipLaunchKernelGGL((reduce_kernel<float, RED_BWD>), dim3(S), dim3(256), 0, stream, M, C, (const float*)y, (const float*)dout, scale, shift, mean, invstd, ws);
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, S, ws, dbeta, dgamma);
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_bwd_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)dout, scale, shift,
                           mean, invstd, gamma, dbeta, dgamma, (bf16_t*)dy);
    else
        hipLaunchKernelGGL(bn_bwd_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const float*)y, (const float*)dout, scale, shift,
                           mean, invstd, gamma, dbeta, dgamma, (float*)dy);
    UIA_CHECK_LAUNCH();
    return 0;
}

// the dropout of one call: off in eval mode and at drop_p == 0
static int drop_of(const char* fn, int training, long n, float drop_p, uint64_t seed, const uint8_t* keep_mask, Drop* d) {
    UIA_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%f outside [0, 1)", fn, drop_p);
    *d = Drop{nullptr, seed, 0u, 1.f, 0};
    if (!training || drop_p == 0.f) return 0;
    UIA_CHECK_ARG(keep_mask || (n % 8 == 0 && n / 8 <= 0xFFFFFFFFl), "%s: the generated mask needs M*C=%ld a multiple of 8 within the generator's 2^35 elements", fn, n);
    *d = Drop{keep_mask, seed, dropout_thresh16(drop_p), 1.0f / (1.0f - drop_p), 1};
    return 0;
}

int uia_bn_act_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const float* gamma, const float* beta,
                          float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean, float* invstd,
                          float* scale, float* shift, float slope, void* out, float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    BN_ARGS_OK("uia_bn_act_fwd");
    UIA_CHECK_ARG(y && gamma && beta && scale && shift && out, "uia_bn_act_fwd: null tensor");
    UIA_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "uia_bn_act_fwd: eps must be > 0 and momentum in [0, 1]");
    UIA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "uia_bn_act_fwd: slope=%f outside [0, 1]", slope);
    Drop d;
    if (drop_of("uia_bn_act_fwd", training, M * C, drop_p, seed, keep_mask, &d)) return -1;
    if (training) {
        UIA_CHECK_ARG(ws && mean && invstd, "uia_bn_act_fwd: training needs ws, mean and invstd");
        UIA_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "uia_bn_act_fwd: running mean and variance come together");
        const int S = slices_for(M);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL((reduce_kernel<bf16_t, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        else
            hipLaunchKernelGGL((reduce_kernel<float, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const float*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        UIA_CHECK_LAUNCH();
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, M, C, S, ws, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                           run_mean, run_var, nbt);
    } else {
        UIA_CHECK_ARG(run_mean && run_var, "uia_bn_act_fwd: eval mode needs the running buffers");
        hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, gamma, beta, run_mean, run_var, eps, scale, shift);
    }
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (drop8_ok(d, n, y, out, nullptr)) {
        const unsigned grid = (unsigned)((n / 8 + 255) / 256);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(bn_act_apply8_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, n, C, (const bf16_t*)y, scale, shift, slope, d, (bf16_t*)out);
        else
            hipLaunchKernelGGL(bn_act_apply8_kernel<float>, dim3(grid), dim3(256), 0, stream, n, C, (const float*)y, scale, shift, slope, d, (float*)out);
        UIA_CHECK_LAUNCH();
        return 0;
    }
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_act_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const bf16_t*)y, scale, shift, slope, d, (bf16_t*)out);
    else
        hipLaunchKernelGGL(bn_act_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const float*)y, scale, shift, slope, d, (float*)out);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_act_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy,
                          float slope, float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    BN_ARGS_OK("uia_bn_act_bwd");
    UIA_CHECK_ARG(y && dout && scale && shift && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_act_bwd: null tensor");
    UIA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "uia_bn_act_bwd: slope=%f outside [0, 1]", slope);
    Drop d;
    if (drop_of("uia_bn_act_bwd", 1, M * C, drop_p, seed, keep_mask, &d)) return -1;
    const int S = slices_for(M);
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(reduce_act_bwd_kernel<bf16_t>, dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)dout, scale, shift, mean, invstd, slope, d, ws);
    else
        hipLaunchKernelGGL(reduce_act_bwd_kernel<float>, dim3(S), dim3(256), 0, stream, M, C, (const float*)y, (const float*)dout, scale, shift, mean, invstd, slope, d, ws);
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, S, ws, dbeta, dgamma);
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (drop8_ok(d, n, y, dout, dy)) {
        const unsigned grid = (unsigned)((n / 8 + 255) / 256);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(bn_act_bwd_apply8_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)dout, scale, shift,
                               mean, invstd, gamma, dbeta, dgamma, slope, d, (bf16_t*)dy);
        else
            hipLaunchKernelGGL(bn_act_bwd_apply8_kernel<float>, dim3(grid), dim3(256), 0, stream, M, C, (const float*)y, (const float*)dout, scale, shift,
                               mean, invstd, gamma, dbeta, dgamma, slope, d, (float*)dy);
        UIA_CHECK_LAUNCH();
        return 0;
    }
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_act_bwd_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)dout, scale, shift,
                           mean, invstd, gamma, dbeta, dgamma, slope, d, (bf16_t*)dy);
    else
        hipLaunchKernelGGL(bn_act_bwd_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const float*)y, (const float*)dout, scale, shift,
                           mean, invstd, gamma, dbeta, dgamma, slope, d, (float*)dy);
    UIA_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------- BatchNorm + residual add + ReLU (the ResNet baseline's BasicBlock tail)
// out = relu(y·scale + shift + r); statistics, running buffers and scale / shift are uia_bn_fwd's (the same launches).  With r null the
// apply is bn_apply_kernel(relu = 1)'s arithmetic: the same bits.  Backward: dz = dout·[out > 0] (out == 0 takes 0, as uia_bn_relu_bwd at
// z == 0), dr = dz in the tensors' dtype, then the training-mode BatchNorm backward on dz with the reductions of reduce_kernel<RED_BWD>.
namespace {

template <typename T>
__global__ __launch_bounds__(256) void bn_add_relu_apply_kernel(long n, int C, const T* __restrict__ y, const T* __restrict__ r, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = fmaf(to_f32(y[i]), scale[c], shift[c]);
    if (r) v += to_f32(r[i]);
    v = v > 0.f ? v : 0.f;
    out[i] = from_f32<T>(v);
}

template <typename T>
__global__ __launch_bounds__(256) void reduce_add_relu_bwd_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ outv, const T* __restrict__ dout,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ ws) {
    __shared__ float red[2][256];
    const int S = gridDim.x, s = blockIdx.x, tid = threadIdx.x;
    const long per = (M + S - 1) / S;
    const long rb = (long)s * per, re = rb + per < M ? rb + per : M;
    const int Cb = C < 256 ? C : 256, RP = 256 / Cb;
    for (int cbase = 0; cbase < C; cbase += Cb) {
        const int c = cbase + tid % Cb, rl = tid / Cb;
        const bool act = rl < RP && c < C;
        float a = 0.f, q = 0.f;
        if (act && rb < re) {
            const float mu = mean[c], is = invstd[c];
            for (long r = rb + rl; r < re; r += RP) {
                const float dz = to_f32(outv[r * C + c]) > 0.f ? to_f32(dout[r * C + c]) : 0.f;
                a += dz;
                q = fmaf(dz, (to_f32(y[r * C + c]) - mu) * is, q);
            }
        }
        red[0][tid] = a;
        red[1][tid] = q;
        __syncthreads();
        if (rl == 0 && c < C) {
            for (int k = 1; k < RP; ++k) {
                a += red[0][tid + k * Cb];
                q += red[1][tid + k * Cb];
            }
            float* o = ws + ((size_t)s * C + c) * 3;
            o[0] = a;
            o[1] = q;
            o[2] = 0.f;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_add_relu_bwd_apply_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ outv, const T* __restrict__ dout,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                    const float* __restrict__ dbeta, const float* __restrict__ dgamma, T* __restrict__ dy,
                                                                    T* __restrict__ dr) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int c = (int)(i % C);
    const T g = dout[i];
    const bool on = to_f32(outv[i]) > 0.f;
    const float dz = on ? to_f32(g) : 0.f;
    if (dr) dr[i] = on ? g : (T)0.f;
    dy[i] = from_f32<T>(bn_bwd_elem(to_f32(y[i]), dz, mean[c], invstd[c], gamma[c], dbeta[c], dgamma[c], 1.0f / (float)M));
}

}  // namespace

int uia_bn_add_relu_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const void* r, const float* gamma,
                               const float* beta, float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean,
                               float* invstd, float* scale, float* shift, void* out) {
    BN_ARGS_OK("uia_bn_add_relu_fwd");
    UIA_CHECK_ARG(y && gamma && beta && scale && shift && out, "uia_bn_add_relu_fwd: null tensor");
    UIA_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, "uia_bn_add_relu_fwd: eps must be > 0 and momentum in [0, 1]");
    if (training) {
        UIA_CHECK_ARG(ws && mean && invstd, "uia_bn_add_relu_fwd: training needs ws, mean and invstd");
        UIA_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "uia_bn_add_relu_fwd: running mean and variance come together");
        const int S = slices_for(M);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL((reduce_kernel<bf16_t, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        else
            hipLaunchKernelGGL((reduce_kernel<float, RED_STATS>), dim3(S), dim3(256), 0, stream, M, C, (const float*)y, nullptr, nullptr, nullptr, nullptr, nullptr, ws);
        UIA_CHECK_LAUNCH();
        hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, M, C, S, ws, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                           run_mean, run_var, nbt);
    } else {
        UIA_CHECK_ARG(run_mean && run_var, "uia_bn_add_relu_fwd: eval mode needs the running buffers");
        hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, gamma, beta, run_mean, run_var, eps, scale, shift);
    }
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_add_relu_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const bf16_t*)y, (const bf16_t*)r, scale, shift,
                           (bf16_t*)out);
    else
        hipLaunchKernelGGL(bn_add_relu_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, C, (const float*)y, (const float*)r, scale, shift,
                           (float*)out);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_add_relu_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* out, const void* dout, const float* mean,
                               const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, void* dr) {
    BN_ARGS_OK("uia_bn_add_relu_bwd");
    UIA_CHECK_ARG(y && out && dout && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_add_relu_bwd: null tensor");
    const int S = slices_for(M);
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(reduce_add_relu_bwd_kernel<bf16_t>, dim3(S), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)out, (const bf16_t*)dout, mean, invstd, ws);
    else
        hipLaunchKernelGGL(reduce_add_relu_bwd_kernel<float>, dim3(S), dim3(256), 0, stream, M, C, (const float*)y, (const float*)out, (const float*)dout, mean, invstd, ws);
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, C, S, ws, dbeta, dgamma);
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(bn_add_relu_bwd_apply_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const bf16_t*)y, (const bf16_t*)out,
                           (const bf16_t*)dout, mean, invstd, gamma, dbeta, dgamma, (bf16_t*)dy, (bf16_t*)dr);
    else
        hipLaunchKernelGGL(bn_add_relu_bwd_apply_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, M, C, (const float*)y, (const float*)out,
                           (const float*)dout, mean, invstd, gamma, dbeta, dgamma, (float*)dy, (float*)dr);
    UIA_CHECK_LAUNCH();
    return 0;
}
