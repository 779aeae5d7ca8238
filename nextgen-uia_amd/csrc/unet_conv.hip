// unet_conv.hip — the convolutions of the DINOv2 UNet decoder on NHWC activations (channels innermost).
//
// Replaces: nn.Conv2d(k=3, pad=1) and nn.ConvTranspose2d(k=2, s=2) of UNetDecoderUpBlock (the reference's
//           src/third_party/dino/dinov2.py:130-152), forward, data gradient and weight gradient.
//
// One implicit GEMM covers every product that carries an output pixel (uia_conv_igemm):
//   D[n][m] = Σ_k W[n][k] · X[m][k]   (+ bias),  m = output pixel, n = output channel, k = tap·Cin + c.
// X is never materialised: each 32-wide K step is one tap of one channel source, gathered straight from the activation with the
// halo zeroed by predicate.  Three gather / scatter modes:
//   UIA_CONV3      3x3, pad 1, stride 1.  Two input sources split along channels (the decoder's cat[a, s] is never written) and two
//                  outputs split at channel N1 (the data gradient writes da and ds apart).  w [N][9][C1 + C2].
//   UIA_CONVT_FWD  ConvTranspose 2x2 s2 forward: one tap, w [4·Cout][Cin] (row n = (2·di + dj)·Cout + o); the result of pixel (y, x),
//                  row n, lands at (2y + di, 2x + dj), channel o, of the [B, 2H, 2W, Cout] output.
//   UIA_CONVT_BWD  its data gradient: output pixel (y, x) of the H×W grid gathers taps (2y + di, 2x + dj) of the 2H×2W gradient;
//                  w [Cin][4][Cout].
//   UIA_CONV1      1x1: one tap, the same pixel, no scatter (the baseline UNet's conv1x1, src/third_party/unet.py:42); w [N][C1].
// bf16: v_mfma_f32_16x16x32_bf16; fp32 (parity mode): v_mfma_f32_16x16x4_f32 (exact fp32 products, k-ordered).  Workgroup tile 64 n × 128 m,
// four waves of 64 × 32, LDS rows padded by 16 B.  The MFMA path needs C1, C2 (or the gradient's Cout) multiples of 8 and N a multiple of 4
// (uia_conv_igemm_form): with multiples of 32 every 32-wide K step is one tap of one source (the first instantiation, unchanged); otherwise
// the tap and the source are decoded per 8-element chunk and the last K step is zero-filled past K = taps·Cin (GEN).  Every other shape (the
// first and last layers' 3 and num_classes channels) takes a direct VALU kernel with the same contract.
//
// Weight gradient (uia_conv_wgrad): G[r][col] = Σ_m P[m][r] · Q[m][col] over the pixels, split in S contiguous pixel ranges whose partial
// products are added in split order by a second launch: no float atomics, two identical calls give identical bits.
//   UIA_CONV3      P = dy [M][N], Q = the 3x3 gather of cat(x1, x2): G = dW [N][9·Cin].
//   UIA_CONVT_FWD  P = the 2x2 gather of dy (r = tap·Cout + o), Q = x [M][Cin]: G = dW [4·Cout][Cin].
//   UIA_CONV1      P = dy [M][N], Q = x [M][C1]: G = dW [N][C1].
// Its MFMA kernel reads 8-element chunks that must stay inside one tap and one source: channel counts and N multiples of 8
// (uia_conv_wgrad_form).
// The bias gradients are column sums of dy (uia_colsum_ordered, unet_bn.hip).
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int TN = 64, TM = 128, KC = 32;

template <typename T> struct Lds { static constexpr int ROW = KC + 16 / (int)sizeof(T); };

struct Geo {
    int mode, B, H, W;      // output pixel grid (CONV3 / CONVT_BWD) or input grid (CONVT_FWD)
    int C1, C2, N, N1, taps;
};

// input pixel of output pixel (b, y, x) for tap t, or -1 in the zero halo; the source grid is H×W (CONV3, CONVT_FWD) or 2H×2W (CONVT_BWD)
__device__ __forceinline__ long src_pixel(const Geo& g, int b, int y, int x, int t) {
    if (g.mode == UIA_CONV3) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) return -1;
        return ((long)b * g.H + yy) * g.W + xx;
    }
    if (g.mode == UIA_CONVT_BWD) return ((long)b * 2 * g.H + 2 * y + (t >> 1)) * (2 * g.W) + 2 * x + (t & 1);
    return ((long)b * g.H + y) * g.W + x;
}

template <typename T>
__device__ __forceinline__ void load_chunk8(const T* p, T (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        *(bf16x8*)v = *(const bf16x8*)p;
    } else {
        *(f32x4_t*)v = *(const f32x4_t*)p;
        *(f32x4_t*)(v + 4) = *(const f32x4_t*)(p + 4);
    }
}
template <typename T>
__device__ __forceinline__ void zero8(T (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (T)0.f;
}
template <typename T>
__device__ __forceinline__ void lds_put8(T* p, const T (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        *(bf16x8*)p = *(const bf16x8*)v;
    } else {
        *(f32x4_t*)p = *(const f32x4_t*)v;
        *(f32x4_t*)(p + 4) = *(const f32x4_t*)(v + 4);
    }
}

// one 32-wide K step of a 16×16 tile: A rows (LDS, row-major in k), B columns (LDS, row-major in k); lane's fragment per MFMA shape
template <typename T>
__device__ __forceinline__ f32x4_t mma_k32(const T* A, const T* Bm, int lane, f32x4_t acc) {
    constexpr int R = Lds<T>::ROW;
    if constexpr (sizeof(T) == 2) {
        const bf16x8 a = *(const bf16x8*)(A + (lane & 15) * R + 8 * (lane >> 4));
        const bf16x8 b = *(const bf16x8*)(Bm + (lane & 15) * R + 8 * (lane >> 4));
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < KC / 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[(lane & 15) * R + 4 * s + (lane >> 4)], Bm[(lane & 15) * R + 4 * s + (lane >> 4)], acc, 0, 0, 0);
        return acc;
    }
}

// GEN = false: C1, C2 multiples of 32.  GEN = true: multiples of 8, tap and source per chunk, zero fill past K.
template <typename T, bool GEN>
__global__ __launch_bounds__(256) void conv_igemm_kernel(Geo g, const T* __restrict__ x1, const T* __restrict__ x2, const T* __restrict__ w,
                                                         const float* __restrict__ bias, T* __restrict__ y1, T* __restrict__ y2) {
    constexpr int R = Lds<T>::ROW;
    __shared__ __attribute__((aligned(16))) T Ws[TN * R];
    __shared__ __attribute__((aligned(16))) T Xs[TM * R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = (long)g.B * g.H * g.W;
    const long m0 = (long)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;
    const int Cin = g.C1 + g.C2, K = g.taps * Cin;

    // this thread's two pixel rows of the X tile and its weight row
    int pb[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long m = m0 + (tid >> 2) + 64 * i;
        pv[i] = m < M;
        const long mm = pv[i] ? m : 0;
        px[i] = (int)(mm % g.W);
        py[i] = (int)((mm / g.W) % g.H);
        pb[i] = (int)(mm / ((long)g.W * g.H));
    }
    const int kq = (tid & 3) * 8;          // this thread's 8 k of the step
    const int wn = n0 + (tid >> 2);
    f32x4_t acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < K; k0 += KC) {
        int t, ld, cs;
        const T* src;
        bool kin = true;                       // this thread's chunk lies inside K (always, when K is a multiple of 32)
        if constexpr (GEN) {
            kin = k0 + kq < K;
            const int k = kin ? k0 + kq : 0;
            t = k / Cin;
            const int c = k - t * Cin;
            const bool first = c < g.C1;
            src = first ? x1 : x2;
            ld = first ? g.C1 : g.C2;
            cs = first ? c : c - g.C1;
        } else {
            t = k0 / Cin;
            const int c0 = k0 - t * Cin;
            const bool first = c0 < g.C1;
            src = first ? x1 : x2;
            ld = first ? g.C1 : g.C2;
            cs = (first ? c0 : c0 - g.C1) + kq;
        }
        T v[2][8], wv[8];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long p = pv[i] && kin ? src_pixel(g, pb[i], py[i], px[i], t) : -1;
            if (p >= 0) load_chunk8(src + p * ld + cs, v[i]);
            else zero8(v[i]);
        }
        if (wn < g.N && kin) load_chunk8(w + (long)wn * K + k0 + kq, wv);
        else zero8(wv);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) lds_put8(Xs + ((tid >> 2) + 64 * i) * R + kq, v[i]);
        lds_put8(Ws + (tid >> 2) * R + kq, wv);
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = mma_k32<T>(Ws + 16 * a * R, Xs + (32 * wave + 16 * b) * R, lane, acc[a][b]);
    }

    // epilogue: lane holds channels n .. n+3 of pixel m (C/D map: column = lane & 15, rows 4·(lane >> 4) + r)
    const int Nout = g.mode == UIA_CONVT_FWD ? g.N / 4 : g.N;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const long m = m0 + 32 * wave + 16 * b + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + 16 * a + 4 * (lane >> 4);
            if (n >= g.N) continue;
            f32x4_t r = acc[a][b];
            int o = n;
            long dst;
            T* out;
            int ldo;
            if (g.mode == UIA_CONVT_FWD) {
                const int t = n / Nout;
                o = n - t * Nout;
                const int xx = (int)(m % g.W), yy = (int)((m / g.W) % g.H), bb = (int)(m / ((long)g.W * g.H));
                dst = ((long)bb * 2 * g.H + 2 * yy + (t >> 1)) * (2 * g.W) + 2 * xx + (t & 1);
                out = y1;
                ldo = Nout;
            } else if (n < g.N1) {
                dst = m; out = y1; ldo = g.N1;
            } else {
                dst = m; out = y2; ldo = g.N - g.N1; o = n - g.N1;
            }
            if (bias) {
                const int ob = g.mode == UIA_CONVT_FWD ? o : n;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] += bias[ob + e];
            }
            store4(out + dst * ldo + o, r);
        }
    }
}

// direct form of the same contract: one thread per (pixel, output channel); any channel counts
template <typename T>
__global__ __launch_bounds__(256) void conv_direct_kernel(Geo g, const T* __restrict__ x1, const T* __restrict__ x2, const T* __restrict__ w,
                                                          const float* __restrict__ bias, T* __restrict__ y1, T* __restrict__ y2) {
    const long M = (long)g.B * g.H * g.W;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * g.N) return;
    const long m = i / g.N;
    const int n = (int)(i - m * g.N);
    const int Cin = g.C1 + g.C2, K = g.taps * Cin;
    const int xx = (int)(m % g.W), yy = (int)((m / g.W) % g.H), bb = (int)(m / ((long)g.W * g.H));
    const T* wr = w + (long)n * K;
    float s = 0.f;
    for (int t = 0; t < g.taps; ++t) {
        const long p = src_pixel(g, bb, yy, xx, t);
        if (p < 0) continue;
        const T* a = x1 + p * g.C1;
        for (int c = 0; c < g.C1; ++c) s = fmaf(to_f32(a[c]), to_f32(wr[t * Cin + c]), s);
        if (g.C2) {
            const T* b2 = x2 + p * g.C2;
            for (int c = 0; c < g.C2; ++c) s = fmaf(to_f32(b2[c]), to_f32(wr[t * Cin + g.C1 + c]), s);
        }
    }
    if (g.mode == UIA_CONVT_FWD) {
        const int Nout = g.N / 4, t = n / Nout, o = n - t * Nout;
        if (bias) s += bias[o];
        y1[(((long)bb * 2 * g.H + 2 * yy + (t >> 1)) * (2 * g.W) + 2 * xx + (t & 1)) * Nout + o] = from_f32<T>(s);
    } else {
        if (bias) s += bias[n];
        if (n < g.N1) y1[m * g.N1 + n] = from_f32<T>(s);
        else y2[m * (g.N - g.N1) + n - g.N1] = from_f32<T>(s);
    }
}

// ---------------------------------------------------------------- weight gradient
// Q[m][col] (A operand, rows = col) and P[m][r] (B operand, columns = r); 8 consecutive elements of one pixel row at a time.
struct WGeo {
    int mode, B, H, W;      // the pixel grid of the reduction: the conv's output grid (CONV3) or the transposed conv's input grid
    int C1, C2, N;          // CONV3: x channels C1 + C2, dy channels N.  CONVT_FWD: x channels C1, dy channels N (= Cout)
    int R, Cols;            // G is R × Cols
    long per;               // pixels per split (multiple of 32)
};

// 8 elements of row m of Q starting at column col (CONV3: 3x3 gather of cat(x1, x2); CONVT: x)
template <typename T>
__device__ __forceinline__ void q_chunk(const WGeo& g, const T* x1, const T* x2, int b, int y, int x, long m, int col, T (&v)[8]) {
    if (g.mode == UIA_CONV3) {
        const int Cin = g.C1 + g.C2, t = col / Cin, c = col - t * Cin;
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) { zero8(v); return; }
        const long p = ((long)b * g.H + yy) * g.W + xx;
        if (c < g.C1) load_chunk8(x1 + p * g.C1 + c, v);
        else load_chunk8(x2 + p * g.C2 + c - g.C1, v);
    } else {
        load_chunk8(x1 + m * g.C1 + col, v);
    }
}
// 8 elements of row m of P starting at column r (CONV3: dy; CONVT: the 2x2 gather of dy, r = tap·Cout + o)
template <typename T>
__device__ __forceinline__ void p_chunk(const WGeo& g, const T* dy, int b, int y, int x, long m, int r, T (&v)[8]) {
    if (g.mode != UIA_CONVT_FWD) {
        load_chunk8(dy + m * g.N + r, v);
    } else {
        const int t = r / g.N, o = r - t * g.N;
        load_chunk8(dy + (((long)b * 2 * g.H + 2 * y + (t >> 1)) * (2 * g.W) + 2 * x + (t & 1)) * g.N + o, v);
    }
}

// workgroup: 64 columns of G (A rows) × 64 rows of G (B columns) over one pixel split; waves take 16 rows of G each
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WGeo g, const T* __restrict__ x1, const T* __restrict__ x2, const T* __restrict__ dy,
                                                         float* __restrict__ out) {
    constexpr int R = Lds<T>::ROW;
    __shared__ __attribute__((aligned(16))) T Qs[64 * R];
    __shared__ __attribute__((aligned(16))) T Ps[64 * R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = (long)g.B * g.H * g.W;
    const int col0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const long mbeg = (long)blockIdx.z * g.per;
    const long mend = mbeg + g.per < M ? mbeg + g.per : M;
    const int lm = tid >> 3, lc = (tid & 7) * 8;    // this thread's pixel of the step and its 8 columns
    const int qc = col0 + lc, pr = r0 + lc;
    f32x4_t acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (long mk = mbeg; mk < mend; mk += 32) {
        const long m = mk + lm;
        T qv[8], pvv[8];
        if (m < mend) {
            const int x = (int)(m % g.W), y = (int)((m / g.W) % g.H), b = (int)(m / ((long)g.W * g.H));
            if (qc < g.Cols) q_chunk(g, x1, x2, b, y, x, m, qc, qv); else zero8(qv);
            if (pr < g.R) p_chunk(g, dy, b, y, x, m, pr, pvv); else zero8(pvv);
        } else {
            zero8(qv);
            zero8(pvv);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Qs[(lc + e) * R + lm] = qv[e];
            Ps[(lc + e) * R + lm] = pvv[e];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = mma_k32<T>(Qs + 16 * a * R, Ps + 16 * wave * R, lane, acc[a]);
    }
    // lane: columns col .. col+3 of G row r
    const int r = r0 + 16 * wave + (lane & 15);
    if (r >= g.R) return;
    float* o = out + (size_t)blockIdx.z * g.R * g.Cols + (size_t)r * g.Cols;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int c = col0 + 16 * a + 4 * (lane >> 4);
        if (c < g.Cols) store4(o + c, acc[a]);
    }
}

// direct weight gradient for any channel counts: 64 outputs × 4 pixel lanes per workgroup, the lanes added in lane order
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_direct_kernel(WGeo g, const T* __restrict__ x1, const T* __restrict__ x2, const T* __restrict__ dy,
                                                                float* __restrict__ out) {
    __shared__ float part[4][64];
    const int tid = threadIdx.x, j = tid & 63, lane4 = tid >> 6;
    const long idx = (long)blockIdx.x * 64 + j;
    const long total = (long)g.R * g.Cols;
    const long M = (long)g.B * g.H * g.W;
    const long mbeg = (long)blockIdx.y * g.per;
    const long mend = mbeg + g.per < M ? mbeg + g.per : M;
    float s = 0.f;
    if (idx < total) {
        const int r = (int)(idx / g.Cols), col = (int)(idx - (long)r * g.Cols);
        const int HW = g.H * g.W;
        for (int m = (int)mbeg + lane4; m < (int)mend; m += 4) {
            const int b = m / HW, r2 = m - b * HW, y = r2 / g.W, x = r2 - y * g.W;
            float q, p;
            if (g.mode == UIA_CONV3) {
                const int Cin = g.C1 + g.C2, t = col / Cin, c = col - t * Cin;
                const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) continue;
                const long pp = ((long)b * g.H + yy) * g.W + xx;
                q = c < g.C1 ? to_f32(x1[pp * g.C1 + c]) : to_f32(x2[pp * g.C2 + c - g.C1]);
                p = to_f32(dy[(long)m * g.N + r]);
            } else if (g.mode == UIA_CONV1) {
                q = to_f32(x1[(long)m * g.C1 + col]);
                p = to_f32(dy[(long)m * g.N + r]);
            } else {
                const int t = r / g.N, o = r - t * g.N;
                q = to_f32(x1[(long)m * g.C1 + col]);
                p = to_f32(dy[(((long)b * 2 * g.H + 2 * y + (t >> 1)) * (2 * g.W) + 2 * x + (t & 1)) * g.N + o]);
            }
            s = fmaf(q, p, s);
        }
    }
    part[lane4][j] = s;
    __syncthreads();
    if (lane4 == 0 && idx < total) out[(size_t)blockIdx.y * total + idx] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
}

// dW = Σ_s ws[s] in split order
__global__ __launch_bounds__(256) void split_sum_kernel(int S, long n, const float* __restrict__ ws, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = ws[i];
    for (int k = 1; k < S; ++k) s += ws[(size_t)k * n + i];
    out[i] = s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// 1: the matrix-core kernel (for 16-byte-aligned operands), 0: the direct kernel.  Pure functions of the shape; the launchers decide by them.
int uia_conv_igemm_form(int mode, int C1, int C2, int N, int N1) {
    if (mode < UIA_CONV3 || mode > UIA_CONV1 || C1 <= 0 || C2 < 0 || N <= 0) return 0;
    return C1 % 8 == 0 && C2 % 8 == 0 && N % 4 == 0 && N1 % 4 == 0 && (mode != UIA_CONVT_FWD || (N / 4) % 4 == 0);
}
int uia_conv_wgrad_form(int mode, int C1, int C2, int N) {
    if ((mode != UIA_CONV3 && mode != UIA_CONVT_FWD && mode != UIA_CONV1) || C1 <= 0 || C2 < 0 || N <= 0) return 0;
    return C1 % 8 == 0 && C2 % 8 == 0 && N % 8 == 0;
}

int uia_conv_igemm_launch(hipStream_t stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N, int N1,
                          const void* w, const float* bias, void* y1, void* y2) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_conv_igemm: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(mode == UIA_CONV3 || mode == UIA_CONVT_FWD || mode == UIA_CONVT_BWD || mode == UIA_CONV1, "uia_conv_igemm: unknown mode %d", mode);
    UIA_CHECK_ARG(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0 && N > 0, "uia_conv_igemm: B=%d H=%d W=%d C1=%d C2=%d N=%d must be positive (C2 >= 0)", B, H, W, C1, C2, N);
    UIA_CHECK_ARG((long)B * H * W * (C1 + C2) * 9 < (1l << 40) && (long)(C1 + C2) * 9 < (1 << 20), "uia_conv_igemm: shape too large");
    UIA_CHECK_ARG(x1 && w && y1, "uia_conv_igemm: null tensor");
    UIA_CHECK_ARG(mode == UIA_CONV3 || C2 == 0, "uia_conv_igemm: the transposed and the 1x1 conv take one source (C2=%d)", C2);
    UIA_CHECK_ARG(C2 == 0 || x2, "uia_conv_igemm: C2=%d with a null second source", C2);
    UIA_CHECK_ARG(mode != UIA_CONVT_FWD || N % 4 == 0, "uia_conv_igemm: transposed conv rows N=%d must be 4·Cout", N);
    if (mode == UIA_CONV3) {
        UIA_CHECK_ARG(N1 > 0 && N1 <= N, "uia_conv_igemm: output split N1=%d outside (0, %d]", N1, N);
        UIA_CHECK_ARG(N1 == N || y2, "uia_conv_igemm: N1=%d < N=%d needs a second output", N1, N);
    } else {
        UIA_CHECK_ARG(N1 == N, "uia_conv_igemm: the transposed and the 1x1 conv have one output (N1 must equal N)");
    }
    const int taps = mode == UIA_CONV3 ? 9 : (mode == UIA_CONVT_BWD ? 4 : 1);
    Geo g{mode, B, H, W, C1, C2, N, N1, taps};
    const long M = (long)B * H * W;
    const size_t es = dtype == UIA_BF16 ? 2 : 4;
    const bool mfma = uia_conv_igemm_form(mode, C1, C2, N, N1) &&
                      aligned16(x1) && aligned16(x2) && aligned16(w) && (((uintptr_t)y1 | (uintptr_t)y2) % (4 * es)) == 0;
    if (mfma) {
        dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((N + TN - 1) / TN));
        const bool gen = C1 % KC != 0 || C2 % KC != 0;
        if (dtype == UIA_BF16) {
            auto k = gen ? conv_igemm_kernel<bf16_t, true> : conv_igemm_kernel<bf16_t, false>;
            hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, g, (const bf16_t*)x1, (const bf16_t*)x2, (const bf16_t*)w, bias, (bf16_t*)y1, (bf16_t*)y2);
        } else {
            auto k = gen ? conv_igemm_kernel<float, true> : conv_igemm_kernel<float, false>;
            hipLaunchKernelGGL(k, grid, dim3(256), 0, stream, g, (const float*)x1, (const float*)x2, (const float*)w, bias, (float*)y1, (float*)y2);
        }
    } else {
        const long n = M * N;
        dim3 grid((unsigned)((n + 255) / 256));
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_direct_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x1, (const bf16_t*)x2, (const bf16_t*)w, bias, (bf16_t*)y1, (bf16_t*)y2);
        else
            hipLaunchKernelGGL(conv_direct_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x1, (const float*)x2, (const float*)w, bias, (float*)y1, (float*)y2);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

static bool wgrad_mfma_shape(int mode, int C1, int C2, int N) { return uia_conv_wgrad_form(mode, C1, C2, N) != 0; }
static int wgrad_rows(int mode, int N) { return mode == UIA_CONVT_FWD ? 4 * N : N; }
static int wgrad_cols(int mode, int C1, int C2) { return mode == UIA_CONV3 ? 9 * (C1 + C2) : C1; }

int uia_conv_wgrad_splits(int mode, int B, int H, int W, int C1, int C2, int N) {
    const long M = (long)B * H * W;
    const int R = wgrad_rows(mode, N);
    const int Cols = wgrad_cols(mode, C1, C2);
    long S;
    if (wgrad_mfma_shape(mode, C1, C2, N)) {
        const long tiles = (long)((Cols + 63) / 64) * ((R + 63) / 64);
        // channel counts below a multiple of 32 are the widest-resolution layers: a handful of tiles over millions of pixels, whose step
        // (gather, two barriers, four MFMAs) is latency-bound, so several workgroups per CU and a higher cap.  The shapes that always
        // ran here keep their split count, and with it their bits.
        const bool narrow = C1 % KC != 0 || C2 % KC != 0;
        const long cap = narrow ? UIA_WGRAD_MAX_NARROW_SPLITS : UIA_WGRAD_MAX_SPLITS;
        S = ((narrow ? 8 : 2) * uia_num_cus() + tiles - 1) / tiles;
        S = S < 1 ? 1 : (S > cap ? cap : S);
    } else {
        // the direct path has few outputs (the last block: 2..4 channels) and a long pixel reduction: spread it over ~8 workgroups per CU
        const long groups = ((long)R * Cols + 63) / 64;
        S = (8 * uia_num_cus() + groups - 1) / groups;
        S = S < 1 ? 1 : (S > UIA_WGRAD_MAX_DIRECT_SPLITS ? UIA_WGRAD_MAX_DIRECT_SPLITS : S);
    }
    const long chunks = (M + 31) / 32;
    if (S > chunks) S = chunks;
    return (int)S;
}

int uia_conv_wgrad_launch(hipStream_t stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N,
                          const void* dy, float* ws, float* dw) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_conv_wgrad: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(mode == UIA_CONV3 || mode == UIA_CONVT_FWD || mode == UIA_CONV1, "uia_conv_wgrad: mode must be UIA_CONV3, UIA_CONVT_FWD or UIA_CONV1 (got %d)", mode);
    UIA_CHECK_ARG(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0 && N > 0, "uia_conv_wgrad: B=%d H=%d W=%d C1=%d C2=%d N=%d must be positive (C2 >= 0)", B, H, W, C1, C2, N);
    UIA_CHECK_ARG(mode == UIA_CONV3 || C2 == 0, "uia_conv_wgrad: the transposed and the 1x1 conv take one source (C2=%d)", C2);
    UIA_CHECK_ARG(x1 && dy && dw && (C2 == 0 || x2), "uia_conv_wgrad: null tensor");
    UIA_CHECK_ARG((long)B * 2 * H * 2 * W < (1l << 31), "uia_conv_wgrad: %ld pixels exceed the 32-bit pixel index", (long)B * H * W);
    const int S = uia_conv_wgrad_splits(mode, B, H, W, C1, C2, N);
    UIA_CHECK_ARG(S == 1 || ws, "uia_conv_wgrad: %d splits need scratch (uia_conv_wgrad_splits · R · Cols floats)", S);
    const long M = (long)B * H * W;
    WGeo g{mode, B, H, W, C1, C2, N, wgrad_rows(mode, N), wgrad_cols(mode, C1, C2), 0};
    g.per = ((M + S - 1) / S + 31) / 32 * 32;
    float* dst = S == 1 ? dw : ws;
    const bool mfma = wgrad_mfma_shape(mode, C1, C2, N) && aligned16(x1) && aligned16(x2) && aligned16(dy) && aligned16(dst);
    if (mfma) {
        dim3 grid((unsigned)((g.Cols + 63) / 64), (unsigned)((g.R + 63) / 64), (unsigned)S);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_wgrad_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x1, (const bf16_t*)x2, (const bf16_t*)dy, dst);
        else
            hipLaunchKernelGGL(conv_wgrad_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x1, (const float*)x2, (const float*)dy, dst);
    } else {
        const long total = (long)g.R * g.Cols;
        dim3 grid((unsigned)((total + 63) / 64), (unsigned)S);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_wgrad_direct_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x1, (const bf16_t*)x2, (const bf16_t*)dy, dst);
        else
            hipLaunchKernelGGL(conv_wgrad_direct_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x1, (const float*)x2, (const float*)dy, dst);
    }
    UIA_CHECK_LAUNCH();
    if (S > 1) {
        const long n = (long)g.R * g.Cols;
        hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, S, n, ws, dw);
        UIA_CHECK_LAUNCH();
    }
    return 0;
}

// ================================================================ strided convolution (the ResNet baseline, src/third_party/resnet.py)
// Conv2d(k, stride s, padding k/2, bias=False), k in {1, 3, 7}, s in {1, 2}, on x [B,H,W,C] -> y [B,Ho,Wo,N], Ho = (H − 1)/s + 1.
// One kernel for the forward and the data gradient: both are D[m][n] = Σ_k Wr[n][k]·Src[m][k] over a destination pixel grid.
//   forward        destination Ho×Wo, N channels; source x; pixel (y, x), tap (ky, kx) reads (s·y + ky − k/2, s·x + kx − k/2).  Wr [N][k²·C].
//   data gradient  destination H×W, C channels; source dy on Ho×Wo; pixel (y, x) takes tap (ky, kx) only where y + k/2 − ky and x + k/2 − kx
//                  are divisible by s and the quotient lies inside Ho×Wo.  Wr [C][k²·N] (column (ky·k + kx)·N + n, taps not flipped).
//                  All k² taps run, the invalid ones as zeros (at s = 2 about three quarters of them).
// The workgroup tile, the LDS layout and the K loop are conv_igemm_kernel<T, true>'s: tap decoded per 8-element chunk, last K step zero-filled.
namespace {

struct SGeo {
    int dgrad;          // 0: forward, 1: data gradient
    int B, Hd, Wd;      // destination pixel grid
    int Hs, Ws;         // source pixel grid
    int Cs, Nd;         // source / destination channels
    int k, s;
};

__device__ __forceinline__ long strided_src_pixel(const SGeo& g, int b, int y, int x, int t) {
    const int ky = t / g.k, kx = t - ky * g.k, h = g.k >> 1;
    int yy, xx;
    if (!g.dgrad) {
        yy = g.s * y + ky - h;
        xx = g.s * x + kx - h;
    } else {
        yy = y + h - ky;
        xx = x + h - kx;
        if (yy < 0 || xx < 0) return -1;
        if (g.s == 2) {
            if ((yy | xx) & 1) return -1;
            yy >>= 1;
            xx >>= 1;
        }
    }
    if (yy < 0 || yy >= g.Hs || xx < 0 || xx >= g.Ws) return -1;
    return ((long)b * g.Hs + yy) * g.Ws + xx;
}

template <typename T>
__global__ __launch_bounds__(256) void conv_strided_kernel(SGeo g, const T* __restrict__ src, const T* __restrict__ w, T* __restrict__ out) {
    constexpr int R = Lds<T>::ROW;
    __shared__ __attribute__((aligned(16))) T Ws[TN * R];
    __shared__ __attribute__((aligned(16))) T Xs[TM * R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = (long)g.B * g.Hd * g.Wd;
    const long m0 = (long)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;
    const int K = g.k * g.k * g.Cs;

    int pb[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long m = m0 + (tid >> 2) + 64 * i;
        pv[i] = m < M;
        const long mm = pv[i] ? m : 0;
        px[i] = (int)(mm % g.Wd);
        py[i] = (int)((mm / g.Wd) % g.Hd);
        pb[i] = (int)(mm / ((long)g.Wd * g.Hd));
    }
    const int kq = (tid & 3) * 8;
    const int wn = n0 + (tid >> 2);
    f32x4_t acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < K; k0 += KC) {
        const bool kin = k0 + kq < K;
        const int kk = kin ? k0 + kq : 0;
        const int t = kk / g.Cs, cs = kk - t * g.Cs;
        T v[2][8], wv[8];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long p = pv[i] && kin ? strided_src_pixel(g, pb[i], py[i], px[i], t) : -1;
            if (p >= 0) load_chunk8(src + p * g.Cs + cs, v[i]);
            else zero8(v[i]);
        }
        if (wn < g.Nd && kin) load_chunk8(w + (long)wn * K + k0 + kq, wv);
        else zero8(wv);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2; ++i) lds_put8(Xs + ((tid >> 2) + 64 * i) * R + kq, v[i]);
        lds_put8(Ws + (tid >> 2) * R + kq, wv);
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = mma_k32<T>(Ws + 16 * a * R, Xs + (32 * wave + 16 * b) * R, lane, acc[a][b]);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const long m = m0 + 32 * wave + 16 * b + (lane & 15);
        if (m >= M) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int n = n0 + 16 * a + 4 * (lane >> 4);
            if (n < g.Nd) store4(out + m * g.Nd + n, acc[a][b]);
        }
    }
}

// direct form of the same contract: one thread per (destination pixel, destination channel); any channel counts, any alignment
template <typename T>
__global__ __launch_bounds__(256) void conv_strided_direct_kernel(SGeo g, const T* __restrict__ src, const T* __restrict__ w, T* __restrict__ out) {
    const long M = (long)g.B * g.Hd * g.Wd;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * g.Nd) return;
    const long m = i / g.Nd;
    const int n = (int)(i - m * g.Nd);
    const int taps = g.k * g.k;
    const int xx = (int)(m % g.Wd), yy = (int)((m / g.Wd) % g.Hd), bb = (int)(m / ((long)g.Wd * g.Hd));
    const T* wr = w + (long)n * taps * g.Cs;
    float s = 0.f;
    for (int t = 0; t < taps; ++t) {
        const long p = strided_src_pixel(g, bb, yy, xx, t);
        if (p < 0) continue;
        const T* a = src + p * g.Cs;
        for (int c = 0; c < g.Cs; ++c) s = fmaf(to_f32(a[c]), to_f32(wr[t * g.Cs + c]), s);
    }
    out[i] = from_f32<T>(s);
}

// weight gradient: G[n][col] = Σ_m dy[m][n]·Q[m][col] over the Ho×Wo output pixels, Q the strided gather of x (col = tap·C + c)
struct SWGeo {
    int B, H, W, Ho, Wo;
    int C, N, k, s;
    int Cols;           // k²·C
    long per;           // output pixels per split (multiple of 32)
};

template <typename T>
__device__ __forceinline__ void strided_q_chunk(const SWGeo& g, const T* x, int b, int y, int xo, int col, T (&v)[8]) {
    const int t = col / g.C, c = col - t * g.C;
    const int ky = t / g.k, kx = t - ky * g.k;
    const int yy = g.s * y + ky - (g.k >> 1), xx = g.s * xo + kx - (g.k >> 1);
    if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) { zero8(v); return; }
    load_chunk8(x + (((long)b * g.H + yy) * g.W + xx) * g.C + c, v);
}

template <typename T>
__global__ __launch_bounds__(256) void conv_strided_wgrad_kernel(SWGeo g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ out) {
    constexpr int R = Lds<T>::ROW;
    __shared__ __attribute__((aligned(16))) T Qs[64 * R];
    __shared__ __attribute__((aligned(16))) T Ps[64 * R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = (long)g.B * g.Ho * g.Wo;
    const int col0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const long mbeg = (long)blockIdx.z * g.per;
    const long mend = mbeg + g.per < M ? mbeg + g.per : M;
    const int lm = tid >> 3, lc = (tid & 7) * 8;
    const int qc = col0 + lc, pr = r0 + lc;
    f32x4_t acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (long mk = mbeg; mk < mend; mk += 32) {
        const long m = mk + lm;
        T qv[8], pvv[8];
        if (m < mend) {
            const int xo = (int)(m % g.Wo), y = (int)((m / g.Wo) % g.Ho), b = (int)(m / ((long)g.Wo * g.Ho));
            if (qc < g.Cols) strided_q_chunk(g, x, b, y, xo, qc, qv); else zero8(qv);
            if (pr < g.N) load_chunk8(dy + m * g.N + pr, pvv); else zero8(pvv);
        } else {
            zero8(qv);
            zero8(pvv);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Qs[(lc + e) * R + lm] = qv[e];
            Ps[(lc + e) * R + lm] = pvv[e];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] = mma_k32<T>(Qs + 16 * a * R, Ps + 16 * wave * R, lane, acc[a]);
    }
    const int r = r0 + 16 * wave + (lane & 15);
    if (r >= g.N) return;
    float* o = out + (size_t)blockIdx.z * g.N * g.Cols + (size_t)r * g.Cols;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int c = col0 + 16 * a + 4 * (lane >> 4);
        if (c < g.Cols) store4(o + c, acc[a]);
    }
}

// direct weight gradient: 64 outputs × 4 pixel lanes per workgroup, the lanes added in lane order (as conv_wgrad_direct_kernel)
template <typename T>
__global__ __launch_bounds__(256) void conv_strided_wgrad_direct_kernel(SWGeo g, const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ out) {
    __shared__ float part[4][64];
    const int tid = threadIdx.x, j = tid & 63, lane4 = tid >> 6;
    const long idx = (long)blockIdx.x * 64 + j;
    const long total = (long)g.N * g.Cols;
    const long M = (long)g.B * g.Ho * g.Wo;
    const long mbeg = (long)blockIdx.y * g.per;
    const long mend = mbeg + g.per < M ? mbeg + g.per : M;
    float s = 0.f;
    if (idx < total) {
        const int r = (int)(idx / g.Cols), col = (int)(idx - (long)r * g.Cols);
        const int t = col / g.C, c = col - t * g.C, ky = t / g.k, kx = t - ky * g.k, h = g.k >> 1;
        const int HW = g.Ho * g.Wo;
        for (int m = (int)mbeg + lane4; m < (int)mend; m += 4) {
            const int b = m / HW, r2 = m - b * HW, y = r2 / g.Wo, xo = r2 - y * g.Wo;
            const int yy = g.s * y + ky - h, xx = g.s * xo + kx - h;
            if (yy < 0 || yy >= g.H || xx < 0 || xx >= g.W) continue;
            s = fmaf(to_f32(x[(((long)b * g.H + yy) * g.W + xx) * g.C + c]), to_f32(dy[(long)m * g.N + r]), s);
        }
    }
    part[lane4][j] = s;
    __syncthreads();
    if (lane4 == 0 && idx < total) out[(size_t)blockIdx.y * total + idx] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
}

bool strided_ks_ok(int k, int s) { return (k == 1 || k == 3 || k == 7) && (s == 1 || s == 2); }

}  // namespace

// 1: the matrix-core kernel (for 16-byte-aligned operands), 0: the direct kernel.  dgrad is 0 (forward) or 1 (data gradient); the rule is the same.
int uia_conv_strided_form(int dgrad, int C, int N, int k, int s) {
    if ((dgrad != 0 && dgrad != 1) || !strided_ks_ok(k, s) || C <= 0 || N <= 0) return 0;
    return C % 8 == 0 && N % 8 == 0;
}
int uia_conv_strided_wgrad_form(int C, int N, int k, int s) {
    if (!strided_ks_ok(k, s) || C <= 0 || N <= 0) return 0;
    return C % 8 == 0 && N % 8 == 0;
}

#define STRIDED_ARGS_OK(fn)                                                                                                                  \
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, fn ": dtype must be UIA_F32 or UIA_BF16");                                        \
    UIA_CHECK_ARG(k == 1 || k == 3 || k == 7, fn ": kernel size k=%d is not 1, 3 or 7", k);                                                \
    UIA_CHECK_ARG(s == 1 || s == 2, fn ": stride s=%d is not 1 or 2", s);                                                                  \
    UIA_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && N > 0, fn ": B=%d H=%d W=%d C=%d N=%d must be positive", B, H, W, C, N);             \
    UIA_CHECK_ARG((long)B * H * W * C * k * k < (1l << 40) && (long)(C > N ? C : N) * k * k < (1 << 20) && (long)B * H * W < (1l << 31), \
                  fn ": shape too large")

int uia_conv_strided_launch(hipStream_t stream, int dtype, int dgrad, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* w,
                            void* y) {
    STRIDED_ARGS_OK("uia_conv_strided");
    UIA_CHECK_ARG(dgrad == 0 || dgrad == 1, "uia_conv_strided: dgrad must be 0 (forward) or 1 (data gradient), got %d", dgrad);
    UIA_CHECK_ARG(x && w && y, "uia_conv_strided: null tensor");
    const int Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
    SGeo g = dgrad ? SGeo{1, B, H, W, Ho, Wo, N, C, k, s} : SGeo{0, B, Ho, Wo, H, W, C, N, k, s};
    const long M = (long)g.B * g.Hd * g.Wd;
    const size_t es = dtype == UIA_BF16 ? 2 : 4;
    const bool mfma = uia_conv_strided_form(dgrad, C, N, k, s) && aligned16(x) && aligned16(w) && ((uintptr_t)y % (4 * es)) == 0;
    if (mfma) {
        dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((g.Nd + TN - 1) / TN));
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_strided_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y);
        else
            hipLaunchKernelGGL(conv_strided_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x, (const float*)w, (float*)y);
    } else {
        const long n = M * g.Nd;
        dim3 grid((unsigned)((n + 255) / 256));
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_strided_direct_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y);
        else
            hipLaunchKernelGGL(conv_strided_direct_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x, (const float*)w, (float*)y);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

// the rule of uia_conv_wgrad_splits on the Ho×Wo pixels, the narrow-channel cap included
int uia_conv_strided_wgrad_splits(int B, int H, int W, int C, int k, int s, int N) {
    if (!strided_ks_ok(k, s) || B <= 0 || H <= 0 || W <= 0 || C <= 0 || N <= 0) return 1;
    const long M = (long)B * ((H - 1) / s + 1) * ((W - 1) / s + 1);
    const int Cols = k * k * C;
    long S;
    if (uia_conv_strided_wgrad_form(C, N, k, s)) {
        const long tiles = (long)((Cols + 63) / 64) * ((N + 63) / 64);
        const bool narrow = C % KC != 0;
        const long cap = narrow ? UIA_WGRAD_MAX_NARROW_SPLITS : UIA_WGRAD_MAX_SPLITS;
        S = ((narrow ? 8 : 2) * uia_num_cus() + tiles - 1) / tiles;
        S = S < 1 ? 1 : (S > cap ? cap : S);
    } else {
        const long groups = ((long)N * Cols + 63) / 64;
        S = (8 * uia_num_cus() + groups - 1) / groups;
        S = S < 1 ? 1 : (S > UIA_WGRAD_MAX_DIRECT_SPLITS ? UIA_WGRAD_MAX_DIRECT_SPLITS : S);
    }
    const long chunks = (M + 31) / 32;
    if (S > chunks) S = chunks;
    return (int)S;
}

int uia_conv_strided_wgrad_launch(hipStream_t stream, int dtype, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* dy,
                                  float* ws, float* dw) {
    STRIDED_ARGS_OK("uia_conv_strided_wgrad");
    UIA_CHECK_ARG(x && dy && dw, "uia_conv_strided_wgrad: null tensor");
    const int S = uia_conv_strided_wgrad_splits(B, H, W, C, k, s, N);
    UIA_CHECK_ARG(S == 1 || ws, "uia_conv_strided_wgrad: %d splits need scratch (uia_conv_strided_wgrad_splits · N · k²·C floats)", S);
    SWGeo g{B, H, W, (H - 1) / s + 1, (W - 1) / s + 1, C, N, k, s, k * k * C, 0};
    const long M = (long)B * g.Ho * g.Wo;
    g.per = ((M + S - 1) / S + 31) / 32 * 32;
    float* dst = S == 1 ? dw : ws;
    const bool mfma = uia_conv_strided_wgrad_form(C, N, k, s) && aligned16(x) && aligned16(dy) && aligned16(dst);
    if (mfma) {
        dim3 grid((unsigned)((g.Cols + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)S);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_strided_wgrad_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x, (const bf16_t*)dy, dst);
        else
            hipLaunchKernelGGL(conv_strided_wgrad_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x, (const float*)dy, dst);
    } else {
        const long total = (long)N * g.Cols;
        dim3 grid((unsigned)((total + 63) / 64), (unsigned)S);
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(conv_strided_wgrad_direct_kernel<bf16_t>, grid, dim3(256), 0, stream, g, (const bf16_t*)x, (const bf16_t*)dy, dst);
        else
            hipLaunchKernelGGL(conv_strided_wgrad_direct_kernel<float>, grid, dim3(256), 0, stream, g, (const float*)x, (const float*)dy, dst);
    }
    UIA_CHECK_LAUNCH();
    if (S > 1) {
        const long n = (long)N * g.Cols;
        hipLaunchKernelGGL(split_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, S, n, ws, dw);
        UIA_CHECK_LAUNCH();
    }
    return 0;
}
