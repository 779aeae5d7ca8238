// decoder.hip — the small kernels of the CLIPSeg decoder (reduce_dim 64, 4 heads of 16, trainable: full backward).
//
// Reference: /root/reference/src/third_party/openai_clip/clipseg_adapter.py:73-98 drives transformers'
// CLIPSegDecoder (third party): reduces → FiLM → three POST-LN layers (d_h = 16, ReLU MLP) →
// Conv3x3 → ReLU → ConvT(k4,s4) → ReLU → ConvT(k4,s4).  The Linear / conv contractions run on gemm.hip + wgrad.hip;
// this file holds what is left.  The decoder is 0.45 GFLOP/image against 35 GFLOP of frozen ViT forward, so these kernels
// are plain VALU, sized for correctness and coalesced access, not for the MFMA roofline.
//
//   attn_small_{fwd,bwd}   softmax(q kᵀ s) v with head dim 16 or 32 (one query per thread, K/V broadcast from LDS)
//   ln_affine_bwd          LayerNorm backward WITH dγ, dβ (decoder LayerNorms are trainable; layernorm.hip is frozen-affine)
//   film_{fwd,bwd}         y = mul[b]·x + add[b]                         (CLIPSegDecoder.forward, conditional_layer)
//   im2col3x3 / col2im3x3  token-major [B,1+hw,C] ↔ [B·hw, 9C] patches of the 3×3 convolution (zero padding 1)
//   unshuffle / shuffle    [B·hw·k², k²(+pad)] GEMM output of the two k=4,s=4 transposed convolutions ↔ [B, hk², wk²]
//   act_bwd                dpre = dy · act′ from the stored post-activation (ReLU) or pre-activation (GELU, QuickGELU)
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------ small-head attention
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_small_fwd_kernel(const UiaAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = p.L;
    float* Ks = (float*)smem;
    float* Vs = Ks + (size_t)L * DH;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
    const size_t row0 = (size_t)b * L;
    const T* qb = (const T*)p.q + row0 * p.ld_qkv + (size_t)h * DH;
    const T* kb = (const T*)p.k + row0 * p.ld_qkv + (size_t)h * DH;
    const T* vb = (const T*)p.v + row0 * p.ld_qkv + (size_t)h * DH;
    for (int i = tid; i < L * DH; i += 256) {
        const int r = i / DH, c = i - r * DH;
        Ks[i] = to_f32(kb[(size_t)r * p.ld_qkv + c]);
        Vs[i] = to_f32(vb[(size_t)r * p.ld_qkv + c]);
    }
    __syncthreads();
    int klen = L;
    if (p.mask_kind == UIA_MASK_KEYPAD && p.keylen) { klen = p.keylen[b]; klen = klen < 1 ? 1 : (klen > L ? L : klen); }
    for (int qi = tid; qi < L; qi += 256) {
        float q[DH], o[DH];
#pragma unroll
        for (int c = 0; c < DH; ++c) { q[c] = to_f32(qb[(size_t)qi * p.ld_qkv + c]) * p.scale; o[c] = 0.f; }
        const int kend = p.mask_kind == UIA_MASK_CAUSAL ? (qi + 1 < klen ? qi + 1 : klen) : klen;
        float m = -INFINITY;
        for (int k = 0; k < kend; ++k) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) s = fmaf(q[c], Ks[k * DH + c], s);
            m = fmaxf(m, s);
        }
        float sum = 0.f;
        for (int k = 0; k < kend; ++k) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) s = fmaf(q[c], Ks[k * DH + c], s);
            const float e = expf(s - m);
            sum += e;
#pragma unroll
            for (int c = 0; c < DH; ++c) o[c] = fmaf(e, Vs[k * DH + c], o[c]);
        }
        const float inv = 1.0f / sum;
        T* orow = (T*)p.out + (row0 + qi) * p.ldo + (size_t)h * DH;
#pragma unroll
        for (int c = 0; c < DH; ++c) orow[c] = from_f32<T>(o[c] * inv);
        if (p.lse) p.lse[((size_t)b * p.H + h) * L + qi] = m + logf(sum);
    }
}

template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_small_bwd_kernel(const UiaAttnParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = p.L;
    float* A = (float*)smem;
    float* Bm = A + (size_t)L * DH;
    float* lse = Bm + (size_t)L * DH;
    float* delta = lse + L;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.H, h = blockIdx.x - b * p.H;
    const size_t row0 = (size_t)b * L;
    const T* qb = (const T*)p.q + row0 * p.ld_qkv + (size_t)h * DH;
    const T* kb = (const T*)p.k + row0 * p.ld_qkv + (size_t)h * DH;
    const T* vb = (const T*)p.v + row0 * p.ld_qkv + (size_t)h * DH;
    const T* gb = (const T*)p.dout + row0 * p.lddo + (size_t)h * DH;
    const T* ob = (const T*)p.out + row0 * p.ldo + (size_t)h * DH;
    int klen = L;
    if (p.mask_kind == UIA_MASK_KEYPAD && p.keylen) { klen = p.keylen[b]; klen = klen < 1 ? 1 : (klen > L ? L : klen); }
    for (int r = tid; r < L; r += 256) {
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < DH; ++c) d = fmaf(to_f32(gb[(size_t)r * p.lddo + c]), to_f32(ob[(size_t)r * p.ldo + c]), d);
        delta[r] = d;
        lse[r] = p.lse[((size_t)b * p.H + h) * L + r];
    }
    for (int i = tid; i < L * DH; i += 256) {
        const int r = i / DH, c = i - r * DH;
        A[i] = to_f32(kb[(size_t)r * p.ld_qkv + c]);
        Bm[i] = to_f32(vb[(size_t)r * p.ld_qkv + c]);
    }
    __syncthreads();
    for (int qi = tid; qi < L; qi += 256) {          // dQ[q] = Σ_k ds·K[k]
        float q[DH], go[DH], dq[DH];
#pragma unroll
        for (int c = 0; c < DH; ++c) { q[c] = to_f32(qb[(size_t)qi * p.ld_qkv + c]); go[c] = to_f32(gb[(size_t)qi * p.lddo + c]); dq[c] = 0.f; }
        const int kend = p.mask_kind == UIA_MASK_CAUSAL ? (qi + 1 < klen ? qi + 1 : klen) : klen;
        const float lq = lse[qi], dq_delta = delta[qi];
        for (int k = 0; k < kend; ++k) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) { s = fmaf(q[c], A[k * DH + c], s); dp = fmaf(go[c], Bm[k * DH + c], dp); }
            const float ds = expf(s * p.scale - lq) * (dp - dq_delta) * p.scale;
#pragma unroll
            for (int c = 0; c < DH; ++c) dq[c] = fmaf(ds, A[k * DH + c], dq[c]);
        }
        T* drow = (T*)p.dq + (row0 + qi) * p.ld_dqkv + (size_t)h * DH;
#pragma unroll
        for (int c = 0; c < DH; ++c) drow[c] = from_f32<T>(dq[c]);
    }
    __syncthreads();
    for (int i = tid; i < L * DH; i += 256) {
        const int r = i / DH, c = i - r * DH;
        A[i] = to_f32(qb[(size_t)r * p.ld_qkv + c]);
        Bm[i] = to_f32(gb[(size_t)r * p.lddo + c]);
    }
    __syncthreads();
    for (int ki = tid; ki < L; ki += 256) {          // dV[k] = Σ_q p·dO[q];  dK[k] = Σ_q ds·Q[q]
        T* vrow = (T*)p.dv + (row0 + ki) * p.ld_dqkv + (size_t)h * DH;
        T* krow = (T*)p.dk + (row0 + ki) * p.ld_dqkv + (size_t)h * DH;
        float kv[DH], vv[DH], dk[DH], dv[DH];
#pragma unroll
        for (int c = 0; c < DH; ++c) { kv[c] = to_f32(kb[(size_t)ki * p.ld_qkv + c]); vv[c] = to_f32(vb[(size_t)ki * p.ld_qkv + c]); dk[c] = 0.f; dv[c] = 0.f; }
        if (ki < klen) {
            const int qstart = p.mask_kind == UIA_MASK_CAUSAL ? ki : 0;
            for (int qi = qstart; qi < L; ++qi) {
                float s = 0.f, dp = 0.f;
#pragma unroll
                for (int c = 0; c < DH; ++c) { s = fmaf(A[qi * DH + c], kv[c], s); dp = fmaf(Bm[qi * DH + c], vv[c], dp); }
                const float pv = expf(s * p.scale - lse[qi]);
                const float ds = pv * (dp - delta[qi]) * p.scale;
#pragma unroll
                for (int c = 0; c < DH; ++c) { dv[c] = fmaf(pv, Bm[qi * DH + c], dv[c]); dk[c] = fmaf(ds, A[qi * DH + c], dk[c]); }
            }
        }
#pragma unroll
        for (int c = 0; c < DH; ++c) { vrow[c] = from_f32<T>(dv[c]); krow[c] = from_f32<T>(dk[c]); }
    }
}

// ------------------------------------------------------------------------------------------ LayerNorm backward with dγ, dβ
template <typename T, int NV>
__global__ __launch_bounds__(256) void ln_affine_bwd_kernel(int M, int D, const T* __restrict__ dy, const float* __restrict__ x,
                                                             const float* __restrict__ gamma, float eps, const float* __restrict__ dres,
                                                             float* __restrict__ dx32, float* __restrict__ g_gamma, float* __restrict__ g_beta) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nv = D >> 2;
    f32x4 a_g[NV], a_b[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) a_g[k] = a_b[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int row = blockIdx.x * 4 + wave; row < M; row += gridDim.x * 4) {
        f32x4 v[NV], d[NV];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = lane + 64 * k;
            const bool ok = c < nv;
            v[k] = ok ? load4(x + (size_t)row * D + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
            d[k] = ok ? load4(dy + (size_t)row * D + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
            s += v[k][0] + v[k][1] + v[k][2] + v[k][3];
        }
        const float mean = wave_sum(s) / D;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = lane + 64 * k;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float t = c < nv ? v[k][e] - mean : 0.f; v[k][e] = t; q = fmaf(t, t, q); }
        }
        const float rstd = rsqrtf(wave_sum(q) / D + eps);
        float sg = 0.f, sgx = 0.f;
        f32x4 g[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = lane + 64 * k;
            const f32x4 w = c < nv ? load4(gamma + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[k][e] *= rstd;                                    // xhat
                a_g[k][e] = fmaf(d[k][e], v[k][e], a_g[k][e]);      // dγ = Σ dy·xhat
                a_b[k][e] += d[k][e];                               // dβ = Σ dy
                g[k][e] = d[k][e] * w[e];
                sg += g[k][e];
                sgx = fmaf(g[k][e], v[k][e], sgx);
            }
        }
        const float mg = wave_sum(sg) / D, mgx = wave_sum(sgx) / D;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = lane + 64 * k;
            if (c < nv) {
                f32x4 o = dres ? load4(dres + (size_t)row * D + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += rstd * (g[k][e] - mg - v[k][e] * mgx);
                store4(dx32 + (size_t)row * D + 4 * c, o);
            }
        }
    }
    float* red = (float*)smem;          // [4 waves][2][D]
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = lane + 64 * k;
        if (c < nv) {
            store4(red + (wave * 2 + 0) * D + 4 * c, a_g[k]);
            store4(red + (wave * 2 + 1) * D + 4 * c, a_b[k]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * D; i += 256) {
        const int qn = i / D, c = i - qn * D;
        const float s = red[(0 * 2 + qn) * D + c] + red[(1 * 2 + qn) * D + c] + red[(2 * 2 + qn) * D + c] + red[(3 * 2 + qn) * D + c];
        atomicAdd((qn == 0 ? g_gamma : g_beta) + c, s);
    }
}

// ------------------------------------------------------------------------------------------ FiLM
__global__ void film_fwd_kernel(int B, int N, int C, const float* __restrict__ x, const float* __restrict__ mul, const float* __restrict__ add, float* __restrict__ y) {
    const size_t total = (size_t)B * N * C / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i * 4;
        const int c = (int)(e % C), b = (int)(e / ((size_t)N * C));
        f32x4 v = load4(x + e);
        const f32x4 m = load4(mul + (size_t)b * C + c), a = load4(add + (size_t)b * C + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(v[k], m[k], a[k]);
        store4(y + e, v);
    }
}
// one block per batch entry; thread = (channel c, row part)
__global__ __launch_bounds__(256) void film_bwd_kernel(int N, int C, const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mul,
                                                        float* __restrict__ dx, float* __restrict__ dmul, float* __restrict__ dadd) {
    __shared__ float red[2][256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lanes = C < 256 ? C : 256, parts = 256 / lanes;
    const int c0 = tid % lanes, part = tid / lanes;
    for (int c = c0; c < C; c += lanes) {
        float sm = 0.f, sa = 0.f;
        const float m = mul[(size_t)b * C + c];
        if (part < parts)
            for (int n = part; n < N; n += parts) {
                const size_t e = ((size_t)b * N + n) * C + c;
                const float g = dy[e];
                sm = fmaf(g, x[e], sm);
                sa += g;
                dx[e] = g * m;
            }
        red[0][tid] = sm; red[1][tid] = sa;
        __syncthreads();
        if (part == 0) {
            for (int q = 1; q < parts; ++q) { sm += red[0][c0 + q * lanes]; sa += red[1][c0 + q * lanes]; }
            dmul[(size_t)b * C + c] = sm;
            dadd[(size_t)b * C + c] = sa;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ 3×3 patches of the token grid
// cols[(b*hw + p)][(ky*3+kx)*C + c] = x[b][tok_off + nbr(p,ky,kx)][c]  (0 outside the grid)
template <typename T>
__global__ void im2col3x3_kernel(int B, int h, int w, int C, int ntok, int tok_off, const float* __restrict__ x, T* __restrict__ cols) {
    const int C4 = C >> 2;
    const size_t total = (size_t)B * h * w * 9 * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const int kk = (int)((i / C4) % 9);
        const size_t prow = i / ((size_t)C4 * 9);
        const int pix = (int)(prow % (h * w)), b = (int)(prow / (h * w));
        const int yy = pix / w + kk / 3 - 1, xx = pix % w + kk % 3 - 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = load4(x + ((size_t)b * ntok + tok_off + yy * w + xx) * C + c);
        store4(cols + prow * 9 * C + (size_t)kk * C + c, v);
    }
}
// dx[b][tok_off + p][c] = Σ_kk dcols[(b, p - off(kk))][kk*C + c]   (gather form, no atomics); rows outside the grid are zeroed
template <typename T>
__global__ void col2im3x3_kernel(int B, int h, int w, int C, int ntok, int tok_off, const T* __restrict__ dcols, float* __restrict__ dx) {
    const int C4 = C >> 2;
    const size_t total = (size_t)B * ntok * C4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) * 4;
        const int tok = (int)((i / C4) % ntok), b = (int)(i / ((size_t)C4 * ntok));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (tok >= tok_off && tok < tok_off + h * w) {                    // tokens past the grid (ntok > tok_off + h·w) are no pixel: zero
            const int pix = tok - tok_off, y = pix / w, xq = pix % w;
#pragma unroll
            for (int kk = 0; kk < 9; ++kk) {
                const int sy = y - (kk / 3 - 1), sx = xq - (kk % 3 - 1);        // the output pixel whose patch slot kk reads (y,x)
                if (sy >= 0 && sy < h && sx >= 0 && sx < w) acc += load4(dcols + ((size_t)b * h * w + sy * w + sx) * 9 * C + (size_t)kk * C + c);
            }
        }
        store4(dx + ((size_t)b * ntok + tok) * C + c, acc);
    }
}

// ------------------------------------------------------------------------------------------ two-level pixel (un)shuffle
// tmp row = ((b*h + y)*w + x)*k1² + i*k1 + j ;  tmp col = i2*k2 + j2 ;  logits[b][(y*k1 + i)*k2 + i2][(x*k1 + j)*k2 + j2]
// One thread per (tmp row, i2): the k2 values tmp[row][i2·k2 .. i2·k2 + k2) are k2 CONSECUTIVE pixels of one logits row, so the row is decomposed once per k2 elements
// and in 32-bit arithmetic (the first version decomposed every element with 64-bit divisions: 129 us for the 6.4 M pixels of 128 images, a tenth of that now).
template <typename T>
__global__ void unshuffle_kernel(int B, int h, int w, int k1, int k2, const T* __restrict__ tmp, long ld, float bias, float* __restrict__ out) {
    const int H = h * k1 * k2, W = w * k1 * k2;
    const unsigned groups = (unsigned)B * h * w * k1 * k1 * k2;                          // (row, i2) pairs
    for (unsigned gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
        const unsigned i2 = gi % k2, row = gi / k2;
        const unsigned j = row % k1, ii = (row / k1) % k1, pix = row / (k1 * k1);
        const unsigned x = pix % w, y = (pix / w) % h, b = pix / (w * h);
        const T* src = tmp + (size_t)row * ld + i2 * k2;
        float* dst = out + ((size_t)b * H + (y * k1 + ii) * k2 + i2) * W + (x * k1 + j) * k2;
        for (int j2 = 0; j2 < k2; ++j2) dst[j2] = to_f32(src[j2]) + bias;
    }
}
template <typename T>
__global__ void shuffle_kernel(int B, int h, int w, int k1, int k2, const float* __restrict__ dout, T* __restrict__ dtmp, long ld) {
    const int H = h * k1 * k2, W = w * k1 * k2;
    const unsigned gpr = (unsigned)((ld + k2 - 1) / k2);                                 // groups of k2 columns per tmp row, padding columns included (they are zeroed)
    const unsigned groups = (unsigned)B * h * w * k1 * k1 * gpr;
    for (unsigned gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
        const unsigned i2 = gi % gpr, row = gi / gpr;
        T* dst = dtmp + (size_t)row * ld + i2 * k2;
        const int ncol = (int)ld - (int)(i2 * k2) < k2 ? (int)ld - (int)(i2 * k2) : k2;
        if (i2 < (unsigned)k2) {
            const unsigned j = row % k1, ii = (row / k1) % k1, pix = row / (k1 * k1);
            const unsigned x = pix % w, y = (pix / w) % h, b = pix / (w * h);
            const float* src = dout + ((size_t)b * H + (y * k1 + ii) * k2 + i2) * W + (x * k1 + j) * k2;
            for (int j2 = 0; j2 < ncol; ++j2) dst[j2] = from_f32<T>(src[j2]);
        } else {
            for (int j2 = 0; j2 < ncol; ++j2) dst[j2] = from_f32<T>(0.f);
        }
    }
}

template <typename T>
__device__ __forceinline__ float act_bwd_one(float g, float yv, int act) {
    if (act == UIA_ACT_RELU) return yv > 0.f ? g : 0.f;                 // y = post-activation
    if (act == UIA_ACT_GELU) return g * dgelu_erf(yv);                  // y = pre-activation
    if (act == UIA_ACT_QUICKGELU) return g * dquick_gelu(yv);           // y = pre-activation
    return g;
}
// VEC elements (16 bytes of bf16, 32 of fp32) per thread and iteration; the launcher takes the scalar form when a pointer or the length does not allow it
template <typename T, int VEC>
__global__ void act_bwd_kernel(size_t n, const T* __restrict__ dy, const T* __restrict__ y, int act, T* __restrict__ out) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    const size_t nv = n / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
        const Pack a = ((const Pack*)dy)[i], b = ((const Pack*)y)[i];
        Pack r;
#pragma unroll
        for (int e = 0; e < VEC; ++e) r.v[e] = from_f32<T>(act_bwd_one<T>(to_f32(a.v[e]), to_f32(b.v[e]), act));
        ((Pack*)out)[i] = r;
    }
}

inline int grid_for(size_t work, int block) {
    size_t g = (work + block - 1) / block;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------
int uia_attn_small_launch(hipStream_t stream, int dtype, const UiaAttnParams& p, bool bwd) {
    UIA_CHECK_ARG(p.dh == 16 || p.dh == 32, "uia_attn: head dim %d unsupported (16, 32 or 64)", p.dh);
    UIA_CHECK_ARG(!p.cu_seqlens, "uia_attn: packed sequences (cu_seqlens) need head dim 64");
    UIA_CHECK_ARG(p.L > 0 && p.L <= 1024 && p.B > 0 && p.H > 0, "uia_attn: bad shape");
    // the same operand contract as the head-dim-64 launchers: a key-padding mask without keylen is refused, not run unmasked,
    // and a backward without lse / dout / gradients fails here instead of dereferencing null on the device
    UIA_CHECK_ARG(p.q && p.k && p.v && p.out, "uia_attn: null tensor");
    UIA_CHECK_ARG(p.mask_kind >= UIA_MASK_NONE && p.mask_kind <= UIA_MASK_KEYPAD, "uia_attn: bad mask kind");
    UIA_CHECK_ARG(p.mask_kind != UIA_MASK_KEYPAD || p.keylen, "uia_attn: key-padding mask needs keylen");
    UIA_CHECK_ARG(!bwd || (p.dout && p.lse && p.dq && p.dk && p.dv), "uia_attn_bwd: null tensor");
    {   // bf16, head dim 16, no mask: the MFMA kernels (attention_dh16.hip).  UIA_ATTN_DH16=0 keeps the scalar kernels below (A/B runs, parity cross-check).
        static const bool mfma = []() { const char* e = getenv("UIA_ATTN_DH16"); return !(e && e[0] == '0'); }();
        if (mfma && uia_attn_dh16_ok(dtype, p)) return uia_attn_dh16_launch(stream, p, bwd);
    }
    const size_t lds = bwd ? ((size_t)2 * p.L * p.dh + 2 * p.L) * 4 : (size_t)2 * p.L * p.dh * 4;
    UIA_CHECK_ARG(lds <= 160 * 1024, "uia_attn: L=%d too long for the small-head path", p.L);
    const dim3 grid(p.B * p.H), block(256);
#define UIA_SMALL(KERN, TT, DD)                                                                                          \
    do {                                                                                                                 \
        UIA_CHECK_HIP(hipFuncSetAttribute((const void*)KERN<TT, DD>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
        hipLaunchKernelGGL((KERN<TT, DD>), grid, block, lds, stream, p);                                                 \
    } while (0)
    if (!bwd) {
        if (dtype == UIA_BF16) { if (p.dh == 16) UIA_SMALL(attn_small_fwd_kernel, bf16_t, 16); else UIA_SMALL(attn_small_fwd_kernel, bf16_t, 32); }
        else { if (p.dh == 16) UIA_SMALL(attn_small_fwd_kernel, float, 16); else UIA_SMALL(attn_small_fwd_kernel, float, 32); }
    } else {
        if (dtype == UIA_BF16) { if (p.dh == 16) UIA_SMALL(attn_small_bwd_kernel, bf16_t, 16); else UIA_SMALL(attn_small_bwd_kernel, bf16_t, 32); }
        else { if (p.dh == 16) UIA_SMALL(attn_small_bwd_kernel, float, 16); else UIA_SMALL(attn_small_bwd_kernel, float, 32); }
    }
#undef UIA_SMALL
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_layernorm_bwd_affine_launch(hipStream_t stream, int dtype, int M, int D, const void* dy, const float* x, const float* gamma, float eps,
                                    const float* dres, float* dx32, float* g_gamma, float* g_beta) {
    UIA_CHECK_ARG(M > 0 && D > 0 && D % 4 == 0 && D <= 1024, "uia_layernorm_bwd_affine: unsupported shape M=%d D=%d", M, D);
    UIA_CHECK_ARG(dy && x && gamma && dx32 && g_gamma && g_beta, "uia_layernorm_bwd_affine: null tensor");
    int blocks = (M + 3) / 4;
    blocks = blocks > 1024 ? 1024 : blocks;
    const size_t lds = (size_t)8 * D * sizeof(float);
    const int nvsel = D <= 256 ? 1 : (D <= 768 ? 3 : 4);
#define UIA_LNA(TT, NVV) hipLaunchKernelGGL((ln_affine_bwd_kernel<TT, NVV>), dim3(blocks), dim3(256), lds, stream, M, D, (const TT*)dy, x, gamma, eps, dres, dx32, g_gamma, g_beta)
    if (dtype == UIA_BF16) { if (nvsel == 1) UIA_LNA(bf16_t, 1); else if (nvsel == 3) UIA_LNA(bf16_t, 3); else UIA_LNA(bf16_t, 4); }
    else if (dtype == UIA_F32) { if (nvsel == 1) UIA_LNA(float, 1); else if (nvsel == 3) UIA_LNA(float, 3); else UIA_LNA(float, 4); }
    else { uia_set_error("uia_layernorm_bwd_affine: bad dtype %d", dtype); return -1; }
#undef UIA_LNA
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_film_fwd_launch(hipStream_t stream, int B, int N, int C, const float* x, const float* mul, const float* add, float* y) {
    UIA_CHECK_ARG(B > 0 && N > 0 && C > 0 && C % 4 == 0 && x && mul && add && y, "uia_film_fwd: bad arguments");
    hipLaunchKernelGGL(film_fwd_kernel, dim3(grid_for((size_t)B * N * C / 4, 256)), dim3(256), 0, stream, B, N, C, x, mul, add, y);
    UIA_CHECK_LAUNCH();
    return 0;
}
int uia_film_bwd_launch(hipStream_t stream, int B, int N, int C, const float* dy, const float* x, const float* mul, float* dx, float* dmul, float* dadd) {
    UIA_CHECK_ARG(B > 0 && N > 0 && C > 0 && (C >= 256 ? C % 256 == 0 : 256 % C == 0) && dy && x && mul && dx && dmul && dadd, "uia_film_bwd: bad arguments (C=%d)", C);
    hipLaunchKernelGGL(film_bwd_kernel, dim3(B), dim3(256), 0, stream, N, C, dy, x, mul, dx, dmul, dadd);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_im2col3x3_launch(hipStream_t stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const float* x, void* cols) {
    UIA_CHECK_ARG(B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && tok_off >= 0 && ntok >= tok_off + h * w && x && cols, "uia_im2col3x3: bad arguments");
    const int g = grid_for((size_t)B * h * w * 9 * C / 4, 256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(im2col3x3_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, B, h, w, C, ntok, tok_off, x, (bf16_t*)cols);
    else if (dtype == UIA_F32) hipLaunchKernelGGL(im2col3x3_kernel<float>, dim3(g), dim3(256), 0, stream, B, h, w, C, ntok, tok_off, x, (float*)cols);
    else { uia_set_error("uia_im2col3x3: bad dtype %d", dtype); return -1; }
    UIA_CHECK_LAUNCH();
    return 0;
}
int uia_col2im3x3_launch(hipStream_t stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const void* dcols, float* dx) {
    UIA_CHECK_ARG(B > 0 && h > 0 && w > 0 && C > 0 && C % 4 == 0 && tok_off >= 0 && ntok >= tok_off + h * w && dcols && dx, "uia_col2im3x3: bad arguments");
    const int g = grid_for((size_t)B * ntok * C / 4, 256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(col2im3x3_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, B, h, w, C, ntok, tok_off, (const bf16_t*)dcols, dx);
    else if (dtype == UIA_F32) hipLaunchKernelGGL(col2im3x3_kernel<float>, dim3(g), dim3(256), 0, stream, B, h, w, C, ntok, tok_off, (const float*)dcols, dx);
    else { uia_set_error("uia_col2im3x3: bad dtype %d", dtype); return -1; }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_unshuffle_launch(hipStream_t stream, int dtype, int B, int h, int w, int k1, int k2, const void* tmp, long ld, float bias, float* out) {
    UIA_CHECK_ARG(B > 0 && h > 0 && w > 0 && k1 > 0 && k2 > 0 && ld >= k2 * k2 && tmp && out, "uia_unshuffle: bad arguments");
    UIA_CHECK_ARG((size_t)B * h * w * k1 * k1 * k2 < ((size_t)1 << 31), "uia_unshuffle: %d x %d x %d pixels x %d x %d sub-pixels exceed the kernel's 32-bit row arithmetic", B, h, w, k1, k2);
    const int g = grid_for((size_t)B * h * w * k1 * k1 * k2, 256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(unshuffle_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, B, h, w, k1, k2, (const bf16_t*)tmp, ld, bias, out);
    else if (dtype == UIA_F32) hipLaunchKernelGGL(unshuffle_kernel<float>, dim3(g), dim3(256), 0, stream, B, h, w, k1, k2, (const float*)tmp, ld, bias, out);
    else { uia_set_error("uia_unshuffle: bad dtype %d", dtype); return -1; }
    UIA_CHECK_LAUNCH();
    return 0;
}
int uia_shuffle_launch(hipStream_t stream, int dtype, int B, int h, int w, int k1, int k2, const float* dout, void* dtmp, long ld) {
    UIA_CHECK_ARG(B > 0 && h > 0 && w > 0 && k1 > 0 && k2 > 0 && ld >= k2 * k2 && dout && dtmp, "uia_shuffle: bad arguments");
    UIA_CHECK_ARG((size_t)B * h * w * k1 * k1 * ((ld + k2 - 1) / k2) < ((size_t)1 << 31), "uia_shuffle: %d x %d x %d pixels x %d x %d sub-pixels exceed the kernel's 32-bit row arithmetic", B, h, w, k1, k2);
    const int g = grid_for((size_t)B * h * w * k1 * k1 * ((ld + k2 - 1) / k2), 256);
    if (dtype == UIA_BF16) hipLaunchKernelGGL(shuffle_kernel<bf16_t>, dim3(g), dim3(256), 0, stream, B, h, w, k1, k2, dout, (bf16_t*)dtmp, ld);
    else if (dtype == UIA_F32) hipLaunchKernelGGL(shuffle_kernel<float>, dim3(g), dim3(256), 0, stream, B, h, w, k1, k2, dout, (float*)dtmp, ld);
    else { uia_set_error("uia_shuffle: bad dtype %d", dtype); return -1; }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_act_bwd_launch(hipStream_t stream, int dtype, size_t n, const void* dy, const void* y, int act, void* out) {
    UIA_CHECK_ARG(n > 0 && dy && y && out && act >= UIA_ACT_NONE && act <= UIA_ACT_RELU, "uia_act_bwd: bad arguments");
    const bool vec = n % 8 == 0 && (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)out) % (dtype == UIA_BF16 ? 16 : 32)) == 0;
    const int g = grid_for(vec ? n / 8 : n, 256);
    if (dtype == UIA_BF16 && vec) hipLaunchKernelGGL((act_bwd_kernel<bf16_t, 8>), dim3(g), dim3(256), 0, stream, n, (const bf16_t*)dy, (const bf16_t*)y, act, (bf16_t*)out);
    else if (dtype == UIA_BF16) hipLaunchKernelGGL((act_bwd_kernel<bf16_t, 1>), dim3(g), dim3(256), 0, stream, n, (const bf16_t*)dy, (const bf16_t*)y, act, (bf16_t*)out);
    else if (dtype == UIA_F32 && vec) hipLaunchKernelGGL((act_bwd_kernel<float, 8>), dim3(g), dim3(256), 0, stream, n, (const float*)dy, (const float*)y, act, (float*)out);
    else if (dtype == UIA_F32) hipLaunchKernelGGL((act_bwd_kernel<float, 1>), dim3(g), dim3(256), 0, stream, n, (const float*)dy, (const float*)y, act, (float*)out);
    else { uia_set_error("uia_act_bwd: bad dtype %d", dtype); return -1; }
    UIA_CHECK_LAUNCH();
    return 0;
}
