// unet_bn.hip — BatchNorm2d on NHWC rows [M = B·H·W, C] with the epilogues of three models, and plain column sums (the convs' bias gradients).
//
//   uia_bn_fwd / uia_bn_relu_bwd              BatchNorm + optional ReLU: UNetDecoderUpBlock of the DINOv2 decoder (the reference's
//                                             src/third_party/dino/dinov2.py:130-152), training and eval mode
//   uia_bn_act_fwd / uia_bn_act_bwd           BatchNorm + LeakyReLU + Dropout: the baseline UNet's ConvBlock (src/third_party/unet.py:10-18);
//                                             with slope 1 and no dropout the ResNet downsample branch
//   uia_bn_add_relu_fwd / uia_bn_add_relu_bwd BatchNorm + residual add + ReLU: the ResNet baseline's BasicBlock tail
//
// One skeleton serves all three.  An entry point differs from the others only in its epilogue policy, a small struct passed to the kernels
// by value that says two things about element i: the output given z = y·scale + shift (fwd), and dz given dout (dz).  Everything else is
// written once:
//   reduce_kernel<T, MODE, P>     the slice reduction: the batch statistics (RED_STATS), column sums (RED_SUM) and Σdz, Σdz·x̂ of policy P (RED_DZ)
//   bn_apply_kernel<T, P>         out = P.fwd(y·scale + shift)
//   bn_bwd_apply_kernel<T, P>     dy = γ·r·(dz − Σdz/M − x̂·Σ(dz·x̂)/M) with dz = P.dz(dout) (bn_bwd_elem)
//   bn_act_apply8_kernel, bn_act_bwd_apply8_kernel: the dropout policy's wide form of the two, eight elements per thread
//   bn_fwd_coeffs                 host: statistics + bn_finalize_kernel in training, bn_eval_coeff_kernel in eval mode
//   bn_bwd_run                    host: reduce, col_finalize_kernel, apply
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

// ---------------------------------------------------------------- dropout of the LeakyReLU policy
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

// ---------------------------------------------------------------- epilogue policies
// fwd(z, i): the output at element i from z = y·scale + shift.  dz(z, dout, i, emit): dz at element i; kDzNeedsZ says whether it reads z (else
// the kernels pass 0 and never touch scale / shift); emit is true in the apply pass, where a policy also writes its own outputs (dr), and
// false in the reduction.  kWide: the policy has eight-element kernels.  The three gates are three expressions on purpose: the ReLU gates
// select (a closed gate gives 0 whatever dout holds), the leaky gate multiplies (slope 0 times inf is NaN, and a zero keeps its sign).
struct NoEpi {                                   // RED_STATS and RED_SUM use neither operation
    static constexpr bool kDzNeedsZ = false;
};

struct ReluEpi {                                 // optional ReLU; the backward is that of relu != 0, z == 0 takes 0
    int relu;
    static constexpr bool kDzNeedsZ = true, kWide = false;
    __device__ __forceinline__ float fwd(float z, long) const { return relu ? (z > 0.f ? z : 0.f) : z; }
    template <typename T> __device__ __forceinline__ float dz(float z, const T* dout, long i, bool) const { return z > 0.f ? to_f32(dout[i]) : 0.f; }
};

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : (slope == 0.f ? 0.f : slope * z); }
// z == 0 takes the slope, as PyTorch's leaky_relu backward
__device__ __forceinline__ float leaky_dz(float z, float g, float slope) { return z > 0.f ? g : g * slope; }

struct LeakyDropEpi {                            // LeakyReLU(slope), then dropout: dz = dout·keep/(1−p)·leaky'(z)
    float slope;
    Drop d;
    static constexpr bool kDzNeedsZ = true, kWide = true;
    __device__ __forceinline__ float fwd(float z, long i) const {
        float v = leaky(z, slope);
        if (d.on) v *= drop_factor(d, i);
        return v;
    }
    template <typename T> __device__ __forceinline__ float dz(float z, const T* dout, long i, bool) const {
        float g = to_f32(dout[i]);
        if (d.on) g *= drop_factor(d, i);
        return leaky_dz(z, g, slope);
    }
};

template <typename T>
struct AddReluEpi {                              // relu(z + r), r may be null; dz = dout·[out > 0] (out == 0 takes 0), dr = dz in the tensors' dtype
    const T* r;                                  // forward
    const T* out;                                // backward: the forward's output
    T* dr;                                       // backward, may be null
    static constexpr bool kDzNeedsZ = false, kWide = false;
    __device__ __forceinline__ float fwd(float z, long i) const {
        if (r) z += to_f32(r[i]);
        return z > 0.f ? z : 0.f;
    }
    __device__ __forceinline__ float dz(float, const T* dout, long i, bool emit) const {
        const T g = to_f32(out[i]) > 0.f ? dout[i] : (T)0.f;
        if (emit && dr) dr[i] = g;
        return to_f32(g);
    }
};

// ---------------------------------------------------------------- the slice reduction
enum { RED_STATS = 0, RED_DZ = 1, RED_SUM = 2 };

// ws[(s·C + c)·3 + {0,1,2}]: RED_STATS {Σ(y−K), Σ(y−K)², K}; RED_DZ {Σdz, Σdz·x̂, 0} with P's dz; RED_SUM {Σy, 0, 0}
template <typename T, int MODE, typename P>
__global__ __launch_bounds__(256) void reduce_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd, P p, float* __restrict__ ws) {
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
            if constexpr (MODE == RED_STATS) K = to_f32(y[rb * C + c]);
            float sc = 0.f, sh = 0.f, mu = 0.f, is = 0.f;
            if constexpr (MODE == RED_DZ) { mu = mean[c]; is = invstd[c]; }
            if constexpr (MODE == RED_DZ && P::kDzNeedsZ) { sc = scale[c]; sh = shift[c]; }
            for (long r = rb + rl; r < re; r += RP) {
                const float v = to_f32(y[r * C + c]);
                if constexpr (MODE == RED_STATS) {
                    const float d = v - K;
                    a += d;
                    q = fmaf(d, d, q);
                } else if constexpr (MODE == RED_DZ) {
                    const float dz = p.dz(P::kDzNeedsZ ? fmaf(v, sc, sh) : 0.f, dout, r * C + c, false);
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

// column sums (RED_SUM) or the two BN backward sums (RED_DZ), slices added in order
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

// ---------------------------------------------------------------- the two apply passes
template <typename T, typename P>
__global__ __launch_bounds__(256) void bn_apply_kernel(long n, int C, const T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, P p, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    out[i] = from_f32<T>(p.fwd(fmaf(to_f32(y[i]), scale[c], shift[c]), i));
}

// the same under dropout: eight consecutive elements per thread, so one draw of the generator serves the eight it covers
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
        v[e] = leaky(fmaf(v[e], scale[c], shift[c]), slope) * k[e];
        if (++c == C) c = 0;
    }
    store8(out + i0, v);
}

// one element of the backward after dz: dy = γ·r·(dz − Σdz/M − x̂·Σ(dz·x̂)/M)
__device__ __forceinline__ float bn_bwd_elem(float v, float dz, float mu, float is, float gamma, float dbeta, float dgamma, float inv) {
    const float xh = (v - mu) * is;
    return gamma * is * (dz - dbeta * inv - xh * dgamma * inv);
}

template <typename T, typename P>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(long M, int C, const T* __restrict__ y, const T* __restrict__ dout, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ dbeta, const float* __restrict__ dgamma,
                                                           P p, T* __restrict__ dy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * C) return;
    const int c = (int)(i % C);
    const float v = to_f32(y[i]);
    float z = 0.f;
    if constexpr (P::kDzNeedsZ) z = fmaf(v, scale[c], shift[c]);
    const float dz = p.dz(z, dout, i, true);
    dy[i] = from_f32<T>(bn_bwd_elem(v, dz, mean[c], invstd[c], gamma[c], dbeta[c], dgamma[c], 1.0f / (float)M));
}

// the same under dropout, eight consecutive elements per thread (see bn_act_apply8_kernel)
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
        const float dz = leaky_dz(fmaf(v[e], scale[c], shift[c]), g[e] * k[e], slope);
        v[e] = bn_bwd_elem(v[e], dz, mean[c], invstd[c], gamma[c], dbeta[c], dgamma[c], inv);
        if (++c == C) c = 0;
    }
    store8(dy + i0, v);
}

// ---------------------------------------------------------------- host
int slices_for(long M) { long s = (M + 255) / 256; return (int)(s < UIA_BN_SLICES ? s : UIA_BN_SLICES); }
dim3 blocks_of(long n) { return dim3((unsigned)((n + 255) / 256)); }

// f(Elem<T>{}) with T the element type that `dtype` names
template <typename T> struct Elem { using type = T; };
template <typename F> void with_elem(int dtype, F&& f) {
    if (dtype == UIA_BF16) f(Elem<bf16_t>{});
    else f(Elem<float>{});
}
#define ELEM_OF(t) typename decltype(t)::type

// scale / shift of the forward's apply: from the batch statistics in training (which also fills mean / invstd and updates the running
// buffers), from the running statistics in eval mode
int bn_fwd_coeffs(const char* fn, hipStream_t stream, int dtype, int training, long M, int C, const void* y, const float* gamma, const float* beta,
                  float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean, float* invstd, float* scale,
                  float* shift) {
    if (training) {
        UIA_CHECK_ARG(ws && mean && invstd, "%s: training needs ws, mean and invstd", fn);
        UIA_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "%s: running mean and variance come together", fn);
        const int S = slices_for(M);
        with_elem(dtype, [&](auto t) {
            using T = ELEM_OF(t);
            hipLaunchKernelGGL((reduce_kernel<T, RED_STATS, NoEpi>), dim3(S), dim3(256), 0, stream, M, C, (const T*)y, nullptr, nullptr, nullptr, nullptr, nullptr, NoEpi{}, ws);
        });
        UIA_CHECK_LAUNCH();
        hipLaunchKernelGGL(bn_finalize_kernel, blocks_of(C), dim3(256), 0, stream, M, C, S, ws, gamma, beta, eps, momentum, mean, invstd, scale, shift,
                           run_mean, run_var, nbt);
    } else {
        UIA_CHECK_ARG(run_mean && run_var, "%s: eval mode needs the running buffers", fn);
        hipLaunchKernelGGL(bn_eval_coeff_kernel, blocks_of(C), dim3(256), 0, stream, C, gamma, beta, run_mean, run_var, eps, scale, shift);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

// out = P.fwd(y·scale + shift), one element per thread; policy(t) makes P for the element type
template <typename MakeP>
int bn_fwd_apply(hipStream_t stream, int dtype, long n, int C, const void* y, const float* scale, const float* shift, void* out, MakeP policy) {
    with_elem(dtype, [&](auto t) {
        using T = ELEM_OF(t);
        auto p = policy(t);
        hipLaunchKernelGGL((bn_apply_kernel<T, decltype(p)>), blocks_of(n), dim3(256), 0, stream, n, C, (const T*)y, scale, shift, p, (T*)out);
    });
    UIA_CHECK_LAUNCH();
    return 0;
}

// the backward of every entry point: Σdz and Σdz·x̂ by slice, the slices added in order into dbeta / dgamma, then dy (and the policy's own
// outputs); wide takes the policy's eight-element apply
template <typename MakeP>
int bn_bwd_run(hipStream_t stream, int dtype, long M, int C, const void* y, const void* dout, const float* scale, const float* shift, const float* mean,
               const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, bool wide, MakeP policy) {
    const int S = slices_for(M);
    with_elem(dtype, [&](auto t) {
        using T = ELEM_OF(t);
        auto p = policy(t);
        hipLaunchKernelGGL((reduce_kernel<T, RED_DZ, decltype(p)>), dim3(S), dim3(256), 0, stream, M, C, (const T*)y, (const T*)dout, scale, shift, mean, invstd, p, ws);
    });
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, blocks_of(C), dim3(256), 0, stream, C, S, ws, dbeta, dgamma);
    UIA_CHECK_LAUNCH();
    const long n = M * C;
    with_elem(dtype, [&](auto t) {
        using T = ELEM_OF(t);
        auto p = policy(t);
        if constexpr (decltype(p)::kWide) {
            if (wide) {
                hipLaunchKernelGGL(bn_act_bwd_apply8_kernel<T>, blocks_of(n / 8), dim3(256), 0, stream, M, C, (const T*)y, (const T*)dout, scale, shift, mean, invstd,
                                   gamma, dbeta, dgamma, p.slope, p.d, (T*)dy);
                return;
            }
        }
        hipLaunchKernelGGL((bn_bwd_apply_kernel<T, decltype(p)>), blocks_of(n), dim3(256), 0, stream, M, C, (const T*)y, (const T*)dout, scale, shift, mean, invstd,
                           gamma, dbeta, dgamma, p, (T*)dy);
    });
    UIA_CHECK_LAUNCH();
    return 0;
}

// the dropout of one call: off in eval mode and at drop_p == 0
int drop_of(const char* fn, int training, long n, float drop_p, uint64_t seed, const uint8_t* keep_mask, Drop* d) {
    UIA_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%f outside [0, 1)", fn, drop_p);
    *d = Drop{nullptr, seed, 0u, 1.f, 0};
    if (!training || drop_p == 0.f) return 0;
    UIA_CHECK_ARG(keep_mask || (n % 8 == 0 && n / 8 <= 0xFFFFFFFFl), "%s: the generated mask needs M*C=%ld a multiple of 8 within the generator's 2^35 elements", fn, n);
    *d = Drop{keep_mask, seed, dropout_thresh16(drop_p), 1.0f / (1.0f - drop_p), 1};
    return 0;
}

}  // namespace

#define BN_ARGS_OK(fn)                                                                                                      \
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, fn ": dtype must be UIA_F32 or UIA_BF16");                       \
    UIA_CHECK_ARG(M > 0 && C > 0 && C <= 65536 && M < (1l << 40), fn ": M=%ld C=%d out of range", (long)M, C)
#define BN_FWD_ARGS_OK(fn)                                                                      \
    BN_ARGS_OK(fn);                                                                             \
    UIA_CHECK_ARG(y && gamma && beta && scale && shift && out, fn ": null tensor");             \
    UIA_CHECK_ARG(eps > 0.f && momentum >= 0.f && momentum <= 1.f, fn ": eps must be > 0 and momentum in [0, 1]")
#define BN_FWD_COEFFS(fn)                                                                                                                     \
    if (int rc = bn_fwd_coeffs(fn, stream, dtype, training, M, C, y, gamma, beta, run_mean, run_var, nbt, momentum, eps, ws, mean, invstd, scale, shift)) \
    return rc

int uia_colsum_ordered_launch(hipStream_t stream, int dtype, long M, int C, const void* y, float* ws, float* out) {
    BN_ARGS_OK("uia_colsum_ordered");
    UIA_CHECK_ARG(y && ws && out, "uia_colsum_ordered: null tensor");
    const int S = slices_for(M);
    with_elem(dtype, [&](auto t) {
        using T = ELEM_OF(t);
        hipLaunchKernelGGL((reduce_kernel<T, RED_SUM, NoEpi>), dim3(S), dim3(256), 0, stream, M, C, (const T*)y, nullptr, nullptr, nullptr, nullptr, nullptr, NoEpi{}, ws);
    });
    UIA_CHECK_LAUNCH();
    hipLaunchKernelGGL(col_finalize_kernel, blocks_of(C), dim3(256), 0, stream, C, S, ws, out, nullptr);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const float* gamma, const float* beta,
                      float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean, float* invstd,
                      float* scale, float* shift, int relu, void* out) {
    BN_FWD_ARGS_OK("uia_bn_fwd");
    BN_FWD_COEFFS("uia_bn_fwd");
    return bn_fwd_apply(stream, dtype, M * C, C, y, scale, shift, out, [&](auto) { return ReluEpi{relu}; });
}

int uia_bn_relu_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                           const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy) {
    BN_ARGS_OK("uia_bn_relu_bwd");
    UIA_CHECK_ARG(y && dout && scale && shift && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_relu_bwd: null tensor");
    return bn_bwd_run(stream, dtype, M, C, y, dout, scale, shift, mean, invstd, gamma, ws, dgamma, dbeta, dy, false, [](auto) { return ReluEpi{1}; });
}

int uia_bn_act_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const float* gamma, const float* beta,
                          float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean, float* invstd,
                          float* scale, float* shift, float slope, void* out, float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    BN_FWD_ARGS_OK("uia_bn_act_fwd");
    UIA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "uia_bn_act_fwd: slope=%f outside [0, 1]", slope);
    LeakyDropEpi p{slope, {}};
    if (drop_of("uia_bn_act_fwd", training, M * C, drop_p, seed, keep_mask, &p.d)) return -1;
    BN_FWD_COEFFS("uia_bn_act_fwd");
    const long n = M * C;
    if (!drop8_ok(p.d, n, y, out, nullptr)) return bn_fwd_apply(stream, dtype, n, C, y, scale, shift, out, [&](auto) { return p; });
    with_elem(dtype, [&](auto t) {
        using T = ELEM_OF(t);
        hipLaunchKernelGGL(bn_act_apply8_kernel<T>, blocks_of(n / 8), dim3(256), 0, stream, n, C, (const T*)y, scale, shift, p.slope, p.d, (T*)out);
    });
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_bn_act_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy,
                          float slope, float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    BN_ARGS_OK("uia_bn_act_bwd");
    UIA_CHECK_ARG(y && dout && scale && shift && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_act_bwd: null tensor");
    UIA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "uia_bn_act_bwd: slope=%f outside [0, 1]", slope);
    LeakyDropEpi p{slope, {}};
    if (drop_of("uia_bn_act_bwd", 1, M * C, drop_p, seed, keep_mask, &p.d)) return -1;
    return bn_bwd_run(stream, dtype, M, C, y, dout, scale, shift, mean, invstd, gamma, ws, dgamma, dbeta, dy, drop8_ok(p.d, M * C, y, dout, dy),
                      [&](auto) { return p; });
}

// Statistics, running buffers and scale / shift are uia_bn_fwd's (the same launches); with r null the apply is ReluEpi{1}'s arithmetic.
int uia_bn_add_relu_fwd_launch(hipStream_t stream, int dtype, int training, long M, int C, const void* y, const void* r, const float* gamma,
                               const float* beta, float* run_mean, float* run_var, int64_t* nbt, float momentum, float eps, float* ws, float* mean,
                               float* invstd, float* scale, float* shift, void* out) {
    BN_FWD_ARGS_OK("uia_bn_add_relu_fwd");
    BN_FWD_COEFFS("uia_bn_add_relu_fwd");
    return bn_fwd_apply(stream, dtype, M * C, C, y, scale, shift, out, [&](auto t) { return AddReluEpi<ELEM_OF(t)>{(const ELEM_OF(t)*)r, nullptr, nullptr}; });
}

int uia_bn_add_relu_bwd_launch(hipStream_t stream, int dtype, long M, int C, const void* y, const void* out, const void* dout, const float* mean,
                               const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, void* dr) {
    BN_ARGS_OK("uia_bn_add_relu_bwd");
    UIA_CHECK_ARG(y && out && dout && mean && invstd && gamma && ws && dgamma && dbeta && dy, "uia_bn_add_relu_bwd: null tensor");
    return bn_bwd_run(stream, dtype, M, C, y, dout, nullptr, nullptr, mean, invstd, gamma, ws, dgamma, dbeta, dy, false,
                      [&](auto t) { return AddReluEpi<ELEM_OF(t)>{nullptr, (const ELEM_OF(t)*)out, (ELEM_OF(t)*)dr}; });
}
