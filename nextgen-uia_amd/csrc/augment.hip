// augment.hip — the training-time augmentation of the reference's dataset modules (src/datasets/segmentation.py:14-156, classification.py:14-151) on the
// device, one launch per batch: uia_augment_batch, and its gathering form uia_augment_gather (the few-shot entries' resident training set: output b is
// made from row `src` of an N-row resident tensor, fp32 or uint8; see the end of this comment).
//
// Every random decision is made on the host (src/datasets/augment.py) and arrives as a program table, int32 [B][14][4]: row 0 of an image is
// (n, with_mask, 0, 0), rows 1 .. n (n <= 13) are (opcode, p0, p1, p2), float parameters as float32 bit patterns.  An image with n == 0 is copied bit for
// bit (image and mask).  Otherwise the image is quantised once, q = rint(255 x) clamped to [0, 255], run through its ops as an 8-bit plane exactly as PIL
// 12.2 computes them on an "L" image, and written back as q / 255; the mask (bytes, never interpreted) follows the geometry ops.
//
//   0 identity
//   1 autocontrast   table[i] = clamp(int(i * s + (-lo * s))), s = 255.0 / (hi - lo) in float64; identity when hi <= lo
//   2 equalize       step = (N - h[last non-zero bin]) / 255; table[i] = min(255, (step / 2 + sum_{j < i} h[j]) / step); identity when fewer than two
//                    bins are occupied or step == 0
//   3 blur           p0 = sigma: THIS BUILD'S definition, the true separable Gaussian: taps k = -r .. r, r = ceil(4 sigma), w_k = exp(-k^2 / (2 sigma^2)) /
//                    sum, replicated edges; rows first into an fp32 plane, then columns; each sum runs k = -r .. r in order (fmaf), rounded half up
//   4 contrast       p0 = v: blend against the solid int(mean + 0.5)
//   5 brightness     p0 = v: blend against black
//   6 sharpness      p0 = v: blend against SMOOTH ([1 1 1; 1 5 1; 1 1 1] / 13, rounded to nearest — never a tie —, border pixels copied)
//   7 posterize      p0 = bits: x & ~(2^(8 - bits) - 1)
//   8 solarize       p0 = thr: x < thr ? x : 255 - x
//   9 crop           (p0, p1, p2) = (i, j, side): the square rows i .. i + side - 1, columns j .. j + side - 1 resized to S x S.  Image: PIL's two-pass
//                    bilinear resample, rows first with a uint8 intermediate, two taps per axis (side <= S), float64 coefficients normalised and rounded
//                    to 22-bit fixed point, clip8((2^21 + sum p k) >> 22).  Mask: nearest, source index int(xo) with xo = a / 2 stepped by a = side / S
//                    in float64 (PIL accumulates the coordinate; the table is built by one thread in that order).  side == S is the identity.
//   10 hflip, 11 vflip
//   blend(d, x, v)   t = d + v * (x - d) in fp32, product and sum rounded separately; t <= 0 -> 0, t >= 255 -> 255, else truncated
//
// One workgroup of 1024 threads per image walks the program; the image lives in two uint8 ping-pong planes of the scratch buffer (an fp32 plane for the
// blur, two more byte planes for the mask), never in LDS: 518 x 518 does not fit.  LDS holds the 256-bin histogram (four copies, one per wave & 3; a thread
// merges runs of equal pixels of its 16-byte chunk into one integer atomic), the lookup table, the blur weights and the resample tables.  __syncthreads()
// separates the ops; a block's global writes are visible to its own later reads behind it.  Byte planes are 16-byte aligned and padded: point ops move 16
// bytes per access; the fp32 input and output use 16-byte accesses where the image's first element is aligned (an operand one element into its buffer
// takes the scalar path).  Integer atomics only.
//
// uia_augment_gather: row 0 of output b is (n, with_mask, src, 0) and block b reads resident row src (any row any number of times, B may exceed N) instead
// of row b; everything behind the read is the code above, so an fp32 source gives what uia_augment_batch gives on the gathered rows.  A uint8 source IS
// the 8-bit plane — rint(255 (u / 255)) = u for every byte in fp32 — so the quantisation pass becomes a byte copy into the first plane and an n == 0 row is
// written as (float)u / 255.0f: both are, bit for bit, uia_augment_batch on rows.float() / 255.  Byte rows start at multiples of S^2 bytes: a row on 16
// bytes moves 16 bytes per access, one on 4 bytes (S = 10) a word, any other (odd S) single bytes; the fp32 output keeps its 16-byte stores where
// its own row is aligned.  The row index is checked on the host (0 <= src < N) and clamped again in the kernel.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

// PIL's C code and Python round every product and every sum.  Device code is compiled with floating-point contraction on, __fmul_rn / __dmul_rn are plain
// operators to the compiler, and the backend fuses a product into the sum that follows it whatever a pragma says: a blend d + v (x - d) as one fma puts 2 %
// of the pixels of a contrast by 1.2 one level off.  mul_rn() hands its product through an empty asm statement, which nothing is fused across.
__device__ __forceinline__ float mul_rn(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ double mul_rn(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

constexpr int AUG_MAX_OPS = 13;
constexpr int AUG_ROWS = AUG_MAX_OPS + 1;
constexpr int AUG_THREADS = 1024;
constexpr int AUG_MIN_S = 8;
constexpr int AUG_MAX_S = 1024;
constexpr int AUG_MAX_B = 65535;
constexpr int AUG_MAX_R = 10;                      // sigma <= 2.5
constexpr int AUG_HCOPIES = 4;

enum { OP_IDENTITY, OP_AUTOCONTRAST, OP_EQUALIZE, OP_BLUR, OP_CONTRAST, OP_BRIGHTNESS, OP_SHARPNESS, OP_POSTERIZE, OP_SOLARIZE, OP_CROP, OP_HFLIP, OP_VFLIP, OP_COUNT };

struct AugLayout {
    size_t table, planes, mplanes, fplane, total, P;
};

AugLayout aug_layout(int B, int S) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    AugLayout l;
    l.P = ((size_t)S * S + 15) & ~(size_t)15;      // bytes of one padded byte plane
    l.table = 0;
    l.planes = up((size_t)B * AUG_ROWS * 4 * sizeof(int32_t));
    l.mplanes = l.planes + up((size_t)B * 2 * l.P);
    l.fplane = l.mplanes + up((size_t)B * 2 * l.P);
    l.total = l.fplane + up((size_t)B * l.P * sizeof(float));
    return l;
}

__device__ __forceinline__ int blend8(int d, int x, float v) {
    const float t = __fadd_rn((float)d, mul_rn(v, (float)(x - d)));
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// f(byte) over the first n bytes of a padded, 16-byte aligned plane, in place, 16 bytes per access (the padding past n is rewritten with f of whatever it held)
template <typename F>
__device__ __forceinline__ void map_plane(uint8_t* plane, int n, F f) {
    const int chunks = (n + 15) >> 4;
    for (int c = threadIdx.x; c < chunks; c += AUG_THREADS) {
        uint4 v = *(const uint4*)(plane + (size_t)c * 16);
        unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned o = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) o |= ((unsigned)f((int)((w[q] >> (8 * e)) & 255u)) & 255u) << (8 * e);
            w[q] = o;
        }
        *(uint4*)(plane + (size_t)c * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// out[i] = f(i) for i < n, eight pixels of a thread in flight at once: the planes an op reads and writes come from one scratch pointer, so in a plain loop
// the compiler keeps every pixel's loads behind the previous pixel's store; here the eight f(i) are evaluated before the first store.  (Worth 3 % of the
// launch: these loops are bound by the NUMBER of byte-wide memory instructions, not by their latency — DESIGN.md §4 "Augmentation".)
template <typename T, typename F>
__device__ __forceinline__ void for_pixels(T* out, int n, F f) {
    constexpr int U = 8;
    for (int base = threadIdx.x; base < n; base += U * AUG_THREADS) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * AUG_THREADS;
            if (i < n) v[u] = f(i);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * AUG_THREADS;
            if (i < n) out[i] = v[u];
        }
    }
}

// The two passes of the blur with R taps either side, R a compile-time constant: the weights sit in registers and the tap loop is unrolled, so a pixel's
// loads are issued together instead of one LDS read and one load per trip of a run-time loop.  w: the weights in LDS, centred at AUG_MAX_R, zero beyond
// the op's own radius r <= R — fmaf(0, p, acc) leaves acc as it is, so a wider R computes the same bits.
template <int R>
__device__ __forceinline__ void blur_passes(const uint8_t* cur, float* fp, uint8_t* nxt, int S, int N, const float* w) {
    float wk[2 * R + 1];
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) wk[k] = w[AUG_MAX_R - R + k];
    for_pixels(fp, N, [&](int i) {
        const int y = i / S, x = i - y * S;
        const uint8_t* row = cur + (size_t)y * S;
        float acc = 0.f;
#pragma unroll
        for (int k = -R; k <= R; ++k) acc = fmaf(wk[k + R], (float)row[min(max(x + k, 0), S - 1)], acc);
        return acc;
    });
    __syncthreads();
    for_pixels(nxt, N, [&](int i) {
        const int y = i / S, x = i - y * S;
        float acc = 0.f;
#pragma unroll
        for (int k = -R; k <= R; ++k) acc = fmaf(wk[k + R], fp[(size_t)min(max(y + k, 0), S - 1) * S + x], acc);
        return (uint8_t)(int)fminf(fmaxf(floorf(acc + 0.5f), 0.f), 255.f);
    });
}

// hist[0][.] = the histogram of the first n bytes of the plane.  Ends behind a barrier.
__device__ void plane_histogram(const uint8_t* plane, int n, unsigned (*hist)[256]) {
    const int tid = threadIdx.x;
    for (int i = tid; i < AUG_HCOPIES * 256; i += AUG_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    unsigned* mine = hist[(tid >> 6) & (AUG_HCOPIES - 1)];
    const int chunks = (n + 15) >> 4;
    for (int c = tid; c < chunks; c += AUG_THREADS) {
        const uint4 v = *(const uint4*)(plane + (size_t)c * 16);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        const int valid = min(16, n - c * 16);
        int prev = -1;
        unsigned run = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int x = (int)((w[e >> 2] >> (8 * (e & 3))) & 255u);
            if (e < valid) {
                if (x == prev) {
                    ++run;
                } else {
                    if (run) atomicAdd(&mine[prev], run);
                    prev = x;
                    run = 1;
                }
            }
        }
        if (run) atomicAdd(&mine[prev], run);
    }
    __syncthreads();
    if (tid < 256) hist[0][tid] += hist[1][tid] + hist[2][tid] + hist[3][tid];
    __syncthreads();
}

__device__ __forceinline__ f32x4 bytes_to_unit(unsigned w) {
    const f32x4 v = {(float)(w & 255u) / 255.0f, (float)((w >> 8) & 255u) / 255.0f, (float)((w >> 16) & 255u) / 255.0f, (float)(w >> 24) / 255.0f};
    return v;
}

// GATHER: block b reads resident row prog[2] of `rows` (else row b).  BYTES: the source is the 8-bit plane itself (else fp32 in [0, 1]).
template <bool GATHER, bool BYTES>
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(int S, int rows, const void* __restrict__ images, const uint8_t* __restrict__ masks,
                                                              const int32_t* __restrict__ table, uint8_t* __restrict__ planes, uint8_t* __restrict__ mplanes,
                                                              float* __restrict__ fplanes, size_t P, float* __restrict__ out_images,
                                                              uint8_t* __restrict__ out_masks) {
    __shared__ unsigned hist[AUG_HCOPIES][256];
    __shared__ unsigned scan[256];
    __shared__ uint8_t lut[256];
    __shared__ float wts[2 * AUG_MAX_R + 1];
    __shared__ int rs_first[AUG_MAX_S], rs_k0[AUG_MAX_S], rs_k1[AUG_MAX_S], rs_near[AUG_MAX_S];
    __shared__ int s_lo, s_hi, s_nz;
    __shared__ unsigned s_sum;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int N = S * S;
    const int32_t* prog = table + b * AUG_ROWS * 4;
    const int n_ops = min(max(prog[0], 0), AUG_MAX_OPS);
    const size_t row = GATHER ? (size_t)min(max(prog[2], 0), rows - 1) : b;
    const float* src = (const float*)images + row * (size_t)N;                     // the fp32 source ...
    const uint8_t* usrc = (const uint8_t*)images + row * (size_t)N;               // ... or the byte source
    float* dst = out_images + b * (size_t)N;
    const uint8_t* msrc = masks ? masks + row * (size_t)N : nullptr;
    uint8_t* mdst = masks ? out_masks + b * (size_t)N : nullptr;
    const bool vec = ((BYTES ? (uintptr_t)dst : ((uintptr_t)src | (uintptr_t)dst)) & 15) == 0;
    const int quads = vec ? N >> 2 : 0;                        // elements 4·quads .. N - 1 go one by one
    const int ualign = !BYTES ? 0 : (((uintptr_t)usrc & 15) == 0 ? 16 : (((uintptr_t)usrc & 3) == 0 ? 4 : 1));

    if (n_ops == 0) {                                           // bit for bit
        if (BYTES) {                                            // ... of rows.float() / 255
            int done = 0;
            if (vec && ualign == 16) {
                const int chunks = N >> 4;
                for (int c = tid; c < chunks; c += AUG_THREADS) {
                    const uint4 v = *(const uint4*)(usrc + 16 * (size_t)c);
                    float* d = dst + 16 * (size_t)c;
                    *(f32x4*)d = bytes_to_unit(v.x);
                    *(f32x4*)(d + 4) = bytes_to_unit(v.y);
                    *(f32x4*)(d + 8) = bytes_to_unit(v.z);
                    *(f32x4*)(d + 12) = bytes_to_unit(v.w);
                }
                done = 16 * chunks;
            } else if (vec && ualign == 4) {
                for (int q = tid; q < quads; q += AUG_THREADS) *(f32x4*)(dst + 4 * (size_t)q) = bytes_to_unit(*(const unsigned*)(usrc + 4 * (size_t)q));
                done = 4 * quads;
            }
            for (int i = done + tid; i < N; i += AUG_THREADS) dst[i] = (float)usrc[i] / 255.0f;
        } else {
            for (int q = tid; q < quads; q += AUG_THREADS) *(f32x4*)(dst + 4 * (size_t)q) = *(const f32x4*)(src + 4 * (size_t)q);
            for (int i = 4 * quads + tid; i < N; i += AUG_THREADS) dst[i] = src[i];
        }
        if (msrc)
            for_pixels(mdst, N, [&](int i) { return msrc[i]; });
        return;
    }

    uint8_t* cur = planes + b * 2 * P;
    uint8_t* nxt = cur + P;
    uint8_t* mfree[2] = {mplanes + b * 2 * P, mplanes + b * 2 * P + P};
    const uint8_t* mcur = msrc;
    int mslot = 0;                                              // the mask plane the next geometry op writes
    float* fp = fplanes + b * P;

    if (BYTES) {                                                // the source is the plane: copied, never rounded (cur is 16-byte aligned)
        int done = 0;
        if (ualign == 16) {
            const int chunks = N >> 4;
            for (int c = tid; c < chunks; c += AUG_THREADS) *(uint4*)(cur + 16 * (size_t)c) = *(const uint4*)(usrc + 16 * (size_t)c);
            done = 16 * chunks;
        } else if (ualign == 4) {
            const int words = N >> 2;
            for (int q = tid; q < words; q += AUG_THREADS) *(unsigned*)(cur + 4 * (size_t)q) = *(const unsigned*)(usrc + 4 * (size_t)q);
            done = 4 * words;
        }
        for (int i = done + tid; i < N; i += AUG_THREADS) cur[i] = usrc[i];
    } else {
        auto quant = [](float x) { return (uint8_t)(int)fminf(fmaxf(rintf(x * 255.0f), 0.f), 255.f); };      // fmaxf(NaN, 0) = 0
        for (int q = tid; q < quads; q += AUG_THREADS) {
            const f32x4 v = *(const f32x4*)(src + 4 * (size_t)q);
            *(unsigned*)(cur + 4 * (size_t)q) = (unsigned)quant(v[0]) | ((unsigned)quant(v[1]) << 8) | ((unsigned)quant(v[2]) << 16) | ((unsigned)quant(v[3]) << 24);
        }
        for (int i = 4 * quads + tid; i < N; i += AUG_THREADS) cur[i] = quant(src[i]);
    }
    __syncthreads();

    for (int o = 0; o < n_ops; ++o) {
        const int code = prog[4 * (o + 1)], p0 = prog[4 * (o + 1) + 1], p1 = prog[4 * (o + 1) + 2], p2 = prog[4 * (o + 1) + 3];
        const float pf = __builtin_bit_cast(float, p0);
        switch (code) {                                         // uniform over the block: every barrier below is reached by all threads or none
        case OP_AUTOCONTRAST: {
            if (tid == 0) {
                s_lo = 256;
                s_hi = -1;
            }
            plane_histogram(cur, N, hist);
            if (tid < 256 && hist[0][tid]) {
                atomicMin(&s_lo, tid);
                atomicMax(&s_hi, tid);
            }
            __syncthreads();
            const int lo = s_lo, hi = s_hi;
            if (hi > lo) {
                if (tid < 256) {
                    const double scale = __ddiv_rn(255.0, (double)(hi - lo));
                    const double offset = mul_rn((double)(-lo), scale);
                    const int ix = (int)__dadd_rn(mul_rn((double)tid, scale), offset);
                    lut[tid] = (uint8_t)min(max(ix, 0), 255);
                }
                __syncthreads();
                map_plane(cur, N, [&](int x) { return (int)lut[x]; });
            }
            break;
        }
        case OP_EQUALIZE: {
            if (tid == 0) {
                s_hi = -1;
                s_nz = 0;
            }
            plane_histogram(cur, N, hist);
            if (tid < 256) {
                scan[tid] = hist[0][tid];
                if (hist[0][tid]) {
                    atomicMax(&s_hi, tid);
                    atomicAdd(&s_nz, 1);
                }
            }
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {                  // inclusive Hillis–Steele scan of the 256 bins
                const unsigned add = (tid < 256 && tid >= d) ? scan[tid - d] : 0u;
                __syncthreads();
                if (tid < 256) scan[tid] += add;
                __syncthreads();
            }
            const unsigned step = s_nz > 1 ? ((unsigned)N - hist[0][s_hi]) / 255u : 0u;
            if (step) {
                if (tid < 256) lut[tid] = (uint8_t)min((step / 2 + scan[tid] - hist[0][tid]) / step, 255u);
                __syncthreads();
                map_plane(cur, N, [&](int x) { return (int)lut[x]; });
            }
            break;
        }
        case OP_CONTRAST: {
            if (tid == 0) s_sum = 0;
            plane_histogram(cur, N, hist);
            if (tid < 256 && hist[0][tid]) atomicAdd(&s_sum, (unsigned)tid * hist[0][tid]);      // <= 255 · 2^20
            __syncthreads();
            const int mean = (int)((2ull * s_sum + (unsigned long long)N) / (2ull * (unsigned long long)N));
            map_plane(cur, N, [&](int x) { return blend8(mean, x, pf); });
            break;
        }
        case OP_BRIGHTNESS:
            map_plane(cur, N, [&](int x) { return blend8(0, x, pf); });
            break;
        case OP_POSTERIZE: {
            const int keep = ~((1 << (8 - min(max(p0, 1), 8))) - 1) & 255;
            map_plane(cur, N, [&](int x) { return x & keep; });
            break;
        }
        case OP_SOLARIZE:
            map_plane(cur, N, [&](int x) { return x < p0 ? x : 255 - x; });
            break;
        case OP_SHARPNESS: {
            for_pixels(nxt, N, [&](int i) {
                const int y = i / S, x = i - y * S;
                const int c = cur[i];
                int d = c;                                       // SMOOTH copies the border
                if (y > 0 && y < S - 1 && x > 0 && x < S - 1) {
                    const uint8_t* r0 = cur + i - S;
                    const uint8_t* r2 = cur + i + S;
                    const int acc = r0[-1] + r0[0] + r0[1] + cur[i - 1] + 5 * c + cur[i + 1] + r2[-1] + r2[0] + r2[1];
                    d = (2 * acc + 13) / 26;
                }
                return (uint8_t)blend8(d, c, pf);
            });
            uint8_t* t = cur;
            cur = nxt;
            nxt = t;
            break;
        }
        case OP_BLUR: {
            const int r = min(max((int)ceilf(4.0f * pf), 0), AUG_MAX_R);
            if (tid <= 2 * AUG_MAX_R) {                          // centred at AUG_MAX_R, zero beyond r
                const float k = (float)(tid - AUG_MAX_R);
                wts[tid] = abs(tid - AUG_MAX_R) <= r ? expf(-(k * k) / (2.0f * pf * pf)) : 0.f;
            }
            __syncthreads();
            float wsum = 0.f;
            for (int k = AUG_MAX_R - r; k <= AUG_MAX_R + r; ++k) wsum += wts[k];      // every thread, the same order: k = -r .. r
            __syncthreads();
            if (tid <= 2 * AUG_MAX_R) wts[tid] = wts[tid] / wsum;
            __syncthreads();
            switch (r) {                                         // sigma in [0.75, 1.25] gives r = 3, 4, 5
            case 3: blur_passes<3>(cur, fp, nxt, S, N, wts); break;
            case 4: blur_passes<4>(cur, fp, nxt, S, N, wts); break;
            case 5: blur_passes<5>(cur, fp, nxt, S, N, wts); break;
            default: blur_passes<AUG_MAX_R>(cur, fp, nxt, S, N, wts); break;
            }
            uint8_t* t = cur;
            cur = nxt;
            nxt = t;
            break;
        }
        case OP_CROP: {
            const int ci = p0, cj = p1, side = p2;
            if (ci < 0 || cj < 0 || side < 1 || side >= S || ci + side > S || cj + side > S) break;      // side == S: the identity
            for (int d = tid; d < S; d += AUG_THREADS) {         // PIL's precompute_coeffs, triangle filter, support 1 (side <= S)
                const double scale = __ddiv_rn((double)side, (double)S);
                const double center = mul_rn((double)d + 0.5, scale);
                int xmin = (int)__dadd_rn(__dadd_rn(center, -1.0), 0.5);
                if (xmin < 0) xmin = 0;
                int xmax = (int)__dadd_rn(__dadd_rn(center, 1.0), 0.5);
                if (xmax > side) xmax = side;
                const int cnt = xmax - xmin;                     // 1 or 2
                double a0 = fabs(__dadd_rn(__dadd_rn((double)xmin, -center), 0.5));
                double w0 = a0 < 1.0 ? __dadd_rn(1.0, -a0) : 0.0, w1 = 0.0;
                if (cnt > 1) {
                    const double a1 = fabs(__dadd_rn(__dadd_rn((double)(xmin + 1), -center), 0.5));
                    w1 = a1 < 1.0 ? __dadd_rn(1.0, -a1) : 0.0;
                }
                const double ww = __dadd_rn(w0, w1);
                if (ww != 0.0) {
                    w0 = __ddiv_rn(w0, ww);
                    w1 = __ddiv_rn(w1, ww);
                }
                rs_first[d] = xmin;
                rs_k0[d] = (int)__dadd_rn(0.5, mul_rn(w0, 4194304.0));
                rs_k1[d] = cnt > 1 ? (int)__dadd_rn(0.5, mul_rn(w1, 4194304.0)) : 0;
            }
            if (mcur && tid == AUG_THREADS - 1) {                // the stepped source coordinate of PIL's nearest scaler: sequential float64 adds
                const double a = __ddiv_rn((double)side, (double)S);
                double xo = mul_rn(a, 0.5);
                for (int d = 0; d < S; ++d) {
                    rs_near[d] = min((int)xo, side - 1);
                    xo = __dadd_rn(xo, a);
                }
            }
            __syncthreads();
            for_pixels(nxt, side * S, [&](int i) {               // rows of the crop: side x S
                const int y = i / S, d = i - y * S;
                const uint8_t* row = cur + (size_t)(ci + y) * S + cj;
                const int f = rs_first[d];
                const int acc = (1 << 21) + row[f] * rs_k0[d] + row[min(f + 1, side - 1)] * rs_k1[d];
                return (uint8_t)min(max(acc >> 22, 0), 255);
            });
            if (mcur) {
                uint8_t* mo = mfree[mslot];
                for_pixels(mo, N, [&](int i) {
                    const int y = i / S, x = i - y * S;
                    return mcur[(size_t)(ci + rs_near[y]) * S + cj + rs_near[x]];
                });
                mcur = mo;
                mslot ^= 1;
            }
            __syncthreads();
            for_pixels(cur, N, [&](int i) {                      // columns: S x S, back into the plane the rows were read from
                const int d = i / S, x = i - d * S;
                const int f = rs_first[d];
                const int acc = (1 << 21) + nxt[(size_t)f * S + x] * rs_k0[d] + nxt[(size_t)min(f + 1, side - 1) * S + x] * rs_k1[d];
                return (uint8_t)min(max(acc >> 22, 0), 255);
            });
            break;
        }
        case OP_HFLIP:
        case OP_VFLIP: {
            uint8_t* mo = mcur ? mfree[mslot] : nullptr;
            auto from = [&](int i) {
                const int y = i / S, x = i - y * S;
                return code == OP_HFLIP ? y * S + (S - 1 - x) : (S - 1 - y) * S + x;
            };
            for_pixels(nxt, N, [&](int i) { return cur[from(i)]; });
            if (mo) for_pixels(mo, N, [&](int i) { return mcur[from(i)]; });
            uint8_t* t = cur;
            cur = nxt;
            nxt = t;
            if (mo) {
                mcur = mo;
                mslot ^= 1;
            }
            break;
        }
        default:                                                // identity (an unknown opcode was refused on the host)
            break;
        }
        __syncthreads();
    }

    for (int q = tid; q < quads; q += AUG_THREADS) {
        *(f32x4*)(dst + 4 * (size_t)q) = bytes_to_unit(*(const unsigned*)(cur + 4 * (size_t)q));
    }
    for (int i = 4 * quads + tid; i < N; i += AUG_THREADS) dst[i] = (float)cur[i] / 255.0f;
    if (mcur)
        for_pixels(mdst, N, [&](int i) { return mcur[i]; });
}

}  // namespace

size_t uia_augment_ws_bytes(int B, int S) {
    if (B < 1 || B > AUG_MAX_B || S < AUG_MIN_S || S > AUG_MAX_S) return 0;
    return aug_layout(B, S).total;
}

namespace {

// Every check of both entry points, before anything is enqueued.  rows == 0: uia_augment_batch (image b is row b of B, fp32); rows >= 1: uia_augment_gather.
int aug_check(const char* who, int rows, int B, int S, int src_dtype, const void* images, const uint8_t* masks, const int32_t* programs, void* ws,
              size_t ws_bytes, float* out_images, uint8_t* out_masks) {
    const bool gather = rows != 0;
    UIA_CHECK_ARG(B >= 1 && B <= AUG_MAX_B && S >= AUG_MIN_S && S <= AUG_MAX_S, "%s: bad shape B=%d S=%d (1 <= B <= %d, %d <= S <= %d)", who, B, S, AUG_MAX_B,
                  AUG_MIN_S, AUG_MAX_S);
    if (gather) {
        UIA_CHECK_ARG(rows >= 1, "%s: a resident set of N=%d rows (N >= 1)", who, rows);
        UIA_CHECK_ARG(src_dtype == 0 || src_dtype == 1, "%s: src_dtype %d (0 fp32, 1 uint8)", who, src_dtype);
    }
    UIA_CHECK_ARG(images && programs && ws && out_images, "%s: null tensor", who);
    UIA_CHECK_ARG((masks == nullptr) == (out_masks == nullptr), "%s: masks and out_masks go together", who);
    const size_t pix = (size_t)S * S, in_rows = gather ? (size_t)rows : (size_t)B, elt = src_dtype == 1 ? 1 : sizeof(float);
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {        // a block reads its source row and writes output b: any overlap is a race
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    UIA_CHECK_ARG(!overlap(images, in_rows * pix * elt, out_images, (size_t)B * pix * sizeof(float)) &&
                      (!masks || !overlap(masks, in_rows * pix, out_masks, (size_t)B * pix)),
                  "%s: the outputs must not be the inputs (the ranges overlap)", who);
    UIA_CHECK_ARG((uintptr_t)ws % 16 == 0 && (uintptr_t)images % elt == 0 && (uintptr_t)out_images % 4 == 0,
                  "%s: the workspace must be 16-byte aligned, the images 4-byte aligned", who);
    const AugLayout l = aug_layout(B, S);
    UIA_CHECK_ARG(ws_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, l.total);
    for (int b = 0; b < B; ++b) {                                  // the whole table is checked before anything is enqueued
        const int32_t* p = programs + (size_t)b * AUG_ROWS * 4;
        UIA_CHECK_ARG(p[0] >= 0 && p[0] <= AUG_MAX_OPS, "%s: image %d has %d ops (0 .. %d)", who, b, p[0], AUG_MAX_OPS);
        if (gather) UIA_CHECK_ARG(p[2] >= 0 && p[2] < rows, "%s: output %d is made from row %d of a resident set of %d rows", who, b, p[2], rows);
        for (int o = 1; o <= p[0]; ++o) {
            const int code = p[4 * o], p0 = p[4 * o + 1], p1 = p[4 * o + 2], p2 = p[4 * o + 3];
            const float pf = __builtin_bit_cast(float, p0);
            UIA_CHECK_ARG(code >= 0 && code < OP_COUNT, "%s: image %d op %d: unknown opcode %d", who, b, o - 1, code);
            if (code == OP_BLUR) UIA_CHECK_ARG(pf >= 0.1f && pf <= 2.5f, "%s: image %d op %d: blur sigma %g outside [0.1, 2.5]", who, b, o - 1, (double)pf);
            if (code == OP_CONTRAST || code == OP_BRIGHTNESS || code == OP_SHARPNESS)
                UIA_CHECK_ARG(pf >= 0.f && pf <= 4.f, "%s: image %d op %d: factor %g outside [0, 4]", who, b, o - 1, (double)pf);
            if (code == OP_POSTERIZE) UIA_CHECK_ARG(p0 >= 1 && p0 <= 8, "%s: image %d op %d: posterize to %d bits (1 .. 8)", who, b, o - 1, p0);
            if (code == OP_SOLARIZE) UIA_CHECK_ARG(p0 >= 0 && p0 <= 256, "%s: image %d op %d: solarize threshold %d (0 .. 256)", who, b, o - 1, p0);
            if (code == OP_CROP)
                UIA_CHECK_ARG(p0 >= 0 && p1 >= 0 && p2 >= 1 && p2 <= S && p0 <= S - p2 && p1 <= S - p2,
                              "%s: image %d op %d: crop (i=%d, j=%d, side=%d) leaves the %d x %d image", who, b, o - 1, p0, p1, p2, S, S);
        }
    }
    return 0;
}

template <bool GATHER, bool BYTES>
int aug_launch(hipStream_t stream, int rows, int B, int S, const void* images, const uint8_t* masks, const int32_t* programs, void* ws, float* out_images,
               uint8_t* out_masks) {
    const AugLayout l = aug_layout(B, S);
    char* base = (char*)ws;
    UIA_CHECK_HIP(hipMemcpyAsync(base + l.table, programs, (size_t)B * AUG_ROWS * 4 * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    augment_kernel<GATHER, BYTES><<<dim3((unsigned)B), dim3(AUG_THREADS), 0, stream>>>(S, rows, images, masks, (const int32_t*)(base + l.table),
                                                                                      (uint8_t*)(base + l.planes), (uint8_t*)(base + l.mplanes),
                                                                                      (float*)(base + l.fplane), l.P, out_images, out_masks);
    UIA_CHECK_LAUNCH();
    return 0;
}

}  // namespace

int uia_augment_batch_launch(hipStream_t stream, int B, int S, const float* images, const uint8_t* masks, const int32_t* programs, void* ws, size_t ws_bytes,
                             float* out_images, uint8_t* out_masks) {
    if (int rc = aug_check("uia_augment_batch", 0, B, S, 0, images, masks, programs, ws, ws_bytes, out_images, out_masks)) return rc;
    return aug_launch<false, false>(stream, B, B, S, images, masks, programs, ws, out_images, out_masks);
}

int uia_augment_gather_launch(hipStream_t stream, int N, int B, int S, int src_dtype, const void* images, const uint8_t* masks, const int32_t* programs,
                              void* ws, size_t ws_bytes, float* out_images, uint8_t* out_masks) {
    UIA_CHECK_ARG(N >= 1, "uia_augment_gather: a resident set of N=%d rows (N >= 1)", N);
    if (int rc = aug_check("uia_augment_gather", N, B, S, src_dtype, images, masks, programs, ws, ws_bytes, out_images, out_masks)) return rc;
    return src_dtype == 1 ? aug_launch<true, true>(stream, N, B, S, images, masks, programs, ws, out_images, out_masks)
                          : aug_launch<true, false>(stream, N, B, S, images, masks, programs, ws, out_images, out_masks);
}
