// seg_native_ens.hip — uia_seg_predict_native_ens: uia_seg_predict_native (seg_native.hip) for an ensemble of K members, one launch per batch.  The members
// are K sets of S x S logits of the same pictures (checkpoints, horizontal / vertical flips of the model's input, or both); the launch un-flips them
// while it reads, upsamples every member to each image's own H x W, turns it into a foreground probability, and writes the mean's thresholded mask, the
// overlay, the mean as a byte map, the members' spread as a byte map, and the statistics.  Conventions, limits and checks are seg_native.hip's.
//
// Per image b, descriptor (src_offset or -1, H, W, mask_out_offset, overlay_out_offset or -1, prob_out_offset or -1, spread_out_offset or -1, 0), native
// pixel (y, x) and member k with flip bits fx = flips >> 2k & 1, fy = flips >> (2k + 1) & 1:
//   L'_c[i][j] = L_c[fy ? S - 1 - i : i][fx ? S - 1 - j : j]               the planes of logits fp32 [K][B][2][S][S] as the model would have seen them unflipped
//   u_0, u_1 from L' exactly as seg_native.hip makes them (the same coordinates, rows first, then columns, a tap of weight exactly 0 left out, every
//   product and sum rounded once in fp32)
//   z_k = u_1 - u_0      p_k = 1 / (1 + expf(-z_k))                         (IEEE division)
//   P = (p_0 + ... + p_{K-1}) / K   summed in member order                 mask = 255 where P > threshold, else 0
//   q = (uint8)(255 P + 0.5f)                                               r = (uint8)(255 (max_k p_k - min_k p_k) + 0.5f)
//   a pixel where any z_k is NaN: mask 0, q 0, r 255.
// Outputs inside `out`: mask H * W bytes, overlay H * W * 3 bytes (g, max(g, mask), g) when src and overlay offsets are both >= 0, q H * W bytes at the
// probability offset and r H * W bytes at the spread offset when given; stats[b] as seg_native.hip's; sums[b] = (sum of q over the pixels whose mask byte
// is 255, sum of r over all pixels), uint64, computed whether or not the maps are stored.  A small launch ahead of the kernel sets stats and sums.
//
// One workgroup of 256 threads makes one contiguous run of at most EN_PIX = 2048 pixels of one image: TR = en_rows(S, W) whole rows where a row fits
// (W <= EN_PIX), else a piece of EN_PIX columns of one row.  A thread owns EN_PPT = 8 pixels of the run and keeps their sum, minimum, maximum and NaN
// flags in registers over the member loop:
//   per member  1. the run's rows' vertical blends of both planes, (v_0, v_1) pairs [TR][S], into LDS (32 KiB, reused by every member): coalesced reads
//                  (forwards, or backwards under a horizontal flip) of the 2 x 2 logit rows a native row needs;
//               2. per owned pixel two 8-byte LDS reads, the horizontal blend, the sigmoid, the three accumulators;
//   then        3. mask, q and r into bytes of LDS (6 KiB), the statistics folded as in seg_native.hip plus two 32-bit sums per workgroup that become two
//                  64-bit global atomics;
//               4. the runs are written from LDS in the aligned dwords that cover them (seg_native.hip's sn_store_run).
// No intermediate reaches HBM.  Deterministic: integer atomics only.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_MIN_S = 8, EN_MAX_S = 1024, EN_MAX_B = 65535, EN_MAX_SIDE = 16384, EN_MAX_K = 16;
constexpr int EN_DESC = 8;
constexpr int EN_TR_MAX = 8;                       // rows of a run, at most
constexpr int EN_BLEND = 4096;                     // (v_0, v_1) pairs of a run's vertical blends: TR * S of them
constexpr int EN_PPT = 8;                          // pixels a thread owns
constexpr int EN_PIX = EN_THREADS * EN_PPT;        // pixels of a run, at most

// rows of a run of an image W <= EN_PIX wide under logits S x S: the same on the host (the grid) and in the kernel
__host__ __device__ inline int en_rows(int S, int W) {
    int tr = EN_BLEND / S < EN_PIX / W ? EN_BLEND / S : EN_PIX / W;
    tr = tr < EN_TR_MAX ? tr : EN_TR_MAX;
    return tr < 1 ? 1 : tr;
}
// runs of an H x W image: row tiles where a row fits a run, else every row in pieces of EN_PIX columns
__host__ __device__ inline unsigned en_tiles(int S, int H, int W) {
    if (W <= EN_PIX) {
        const int tr = en_rows(S, W);
        return (unsigned)((H + tr - 1) / tr);
    }
    return (unsigned)H * (unsigned)((W + EN_PIX - 1) / EN_PIX);
}

// the arithmetic of seg_native.hip, statement for statement: u_0 and u_1 must be its values
__device__ __forceinline__ float en_mul(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ __forceinline__ void en_coord(float scale, int i, int S, int& i0, int& i1, float& l) {
    float s = en_mul(scale, (float)i + 0.5f) - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    i0 = min((int)s, S - 1);
    i1 = min(i0 + 1, S - 1);
    l = s - (float)i0;
}
__device__ __forceinline__ float en_blend(float a, float b, float l) {
    return l == 0.0f ? a : en_mul(1.0f - l, a) + en_mul(l, b);
}
__device__ __forceinline__ unsigned en_byte(float v) { return (unsigned)(en_mul(255.0f, v) + 0.5f); }      // v in [0, 1]

template <typename F>
__device__ __forceinline__ void en_store_run(uint8_t* dst, int n, F f) {
    const int a = (int)((uintptr_t)dst & 3u);      // the run starts `a` bytes into its first dword
    const int words = (n + a + 3) >> 2;
    for (int k = threadIdx.x; k < words; k += EN_THREADS) {
        const int j = 4 * k - a;                   // the run's byte at the dword's first address
        if (j >= 0 && j + 4 <= n) {
            const unsigned w = f(j) | (f(j + 1) << 8) | (f(j + 2) << 16) | (f(j + 3) << 24);
            *(unsigned*)(dst + j) = w;
        } else {
            for (int e = 0; e < 4; ++e)
                if (j + e >= 0 && j + e < n) dst[j + e] = (uint8_t)f(j + e);
        }
    }
}

__global__ __launch_bounds__(EN_THREADS) void ens_init_kernel(int n, int32_t* __restrict__ stats, int m, unsigned long long* __restrict__ sums) {
    const int i = blockIdx.x * EN_THREADS + threadIdx.x;
    if (i < n) {
        const int w = i & (EN_DESC - 1);
        stats[i] = (w == 1 || w == 2) ? INT_MAX : ((w == 3 || w == 4) ? -1 : 0);
    }
    if (sums != nullptr && i < m) sums[i] = 0ull;
}

__global__ __launch_bounds__(EN_THREADS) void seg_native_ens_kernel(int K, int S, unsigned flips, float threshold, size_t member, const float* __restrict__ logits,
                                                                    const uint8_t* __restrict__ src, uint8_t* __restrict__ out, const int32_t* __restrict__ desc,
                                                                    int32_t* __restrict__ stats, unsigned long long* __restrict__ sums) {
    __shared__ float2 blend[EN_BLEND];
    __shared__ uint8_t pix[3][EN_PIX];             // mask, q, r
    __shared__ int st[5];
    __shared__ unsigned sm[2];

    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int32_t* d = desc + b * EN_DESC;
    const int soff = d[0], H = d[1], W = d[2], moff = d[3], ooff = d[4], poff = d[5], roff = d[6];
    int row0, rows, col0, cols;                    // the run: `rows` whole rows, or `cols` columns of one row
    if (W <= EN_PIX) {
        const int TR = en_rows(S, W);
        row0 = blockIdx.x * TR;
        if (row0 >= H) return;                     // (uniform over the workgroup: nobody waits at a barrier below)
        rows = min(TR, H - row0);
        col0 = 0;
        cols = W;
    } else {
        const int pieces = (W + EN_PIX - 1) / EN_PIX;
        row0 = blockIdx.x / pieces;
        if (row0 >= H) return;
        rows = 1;
        col0 = (blockIdx.x - row0 * pieces) * EN_PIX;
        cols = min(EN_PIX, W - col0);
    }
    const int n = rows * cols;                     // <= EN_PIX
    const float scale_y = __fdiv_rn((float)S, (float)H), scale_x = __fdiv_rn((float)S, (float)W);      // IEEE division, not a reciprocal

    if (tid == 0) {
        st[0] = 0;
        st[1] = st[2] = INT_MAX;
        st[3] = st[4] = -1;
        sm[0] = sm[1] = 0u;
    }

    int x0[EN_PPT], x1[EN_PPT], base[EN_PPT];      // per owned pixel: its two columns and the start of its row in `blend`
    float lx[EN_PPT], sum[EN_PPT], lo[EN_PPT], hi[EN_PPT];
    unsigned nan = 0u;
#pragma unroll
    for (int e = 0; e < EN_PPT; ++e) {
        const int i = tid + e * EN_THREADS;
        const int r = i / cols, x = col0 + (i - r * cols);
        en_coord(scale_x, x, S, x0[e], x1[e], lx[e]);
        base[e] = r * S;
        sum[e] = 0.0f;
        lo[e] = 1.0f;
        hi[e] = 0.0f;
    }

    for (int k = 0; k < K; ++k) {
        const bool fx = (flips >> (2 * k)) & 1u, fy = (flips >> (2 * k + 1)) & 1u;
        const float* L0 = logits + (size_t)k * member + b * 2 * (size_t)S * S;
        const float* L1 = L0 + (size_t)S * S;
        if (k) __syncthreads();                    // the member before has been read
        for (int i = tid; i < rows * S; i += EN_THREADS) {                       // 1. vertical blends of the un-flipped planes
            const int r = i / S, j = i - r * S;
            int y0, y1;
            float ly;
            en_coord(scale_y, row0 + r, S, y0, y1, ly);
            const size_t c = fx ? S - 1 - j : j, a0 = (size_t)(fy ? S - 1 - y0 : y0) * S + c, a1 = (size_t)(fy ? S - 1 - y1 : y1) * S + c;
            float2 v;
            v.x = en_blend(L0[a0], L0[a1], ly);
            v.y = en_blend(L1[a0], L1[a1], ly);
            blend[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EN_PPT; ++e) {                                       // 2. horizontal blends, the member's probability
            if (tid + e * EN_THREADS < n) {
                const float2 va = blend[base[e] + x0[e]], vb = blend[base[e] + x1[e]];
                const float z = en_blend(va.y, vb.y, lx[e]) - en_blend(va.x, vb.x, lx[e]);
                const float p = __fdiv_rn(1.0f, 1.0f + expf(-z));
                if (z != z) nan |= 1u << e;
                sum[e] += p;
                lo[e] = fminf(lo[e], p);
                hi[e] = fmaxf(hi[e], p);
            }
        }
    }

    int cnt = 0, ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1;
    unsigned sq = 0u, sr = 0u;
    const float fk = (float)K;
#pragma unroll
    for (int e = 0; e < EN_PPT; ++e) {                                           // 3. the bytes and the statistics
        const int i = tid + e * EN_THREADS;
        if (i < n) {
            unsigned m = 0u, q = 0u, r = 255u;     // a NaN member
            if (!((nan >> e) & 1u)) {
                const float P = __fdiv_rn(sum[e], fk);
                m = P > threshold ? 255u : 0u;
                q = en_byte(P);
                r = en_byte(hi[e] - lo[e]);
            }
            pix[0][i] = (uint8_t)m;
            pix[1][i] = (uint8_t)q;
            pix[2][i] = (uint8_t)r;
            sr += r;
            if (m) {
                const int rr = i / cols, y = row0 + rr, x = col0 + (i - rr * cols);
                sq += q;
                ++cnt;
                ymin = min(ymin, y);
                ymax = max(ymax, y);
                xmin = min(xmin, x);
                xmax = max(xmax, x);
            }
        }
    }
    if (cnt) {
        atomicAdd(&st[0], cnt);
        atomicMin(&st[1], ymin);
        atomicMin(&st[2], xmin);
        atomicMax(&st[3], ymax);
        atomicMax(&st[4], xmax);
        atomicAdd(&sm[0], sq);                     // at most EN_PIX * 255: 32 bits hold a workgroup's sums
    }
    if (sr) atomicAdd(&sm[1], sr);
    __syncthreads();

    if (tid == 0) {
        if (st[0]) {
            int32_t* s = stats + b * EN_DESC;
            atomicAdd(&s[0], st[0]);
            atomicMin(&s[1], st[1]);
            atomicMin(&s[2], st[2]);
            atomicMax(&s[3], st[3]);
            atomicMax(&s[4], st[4]);
        }
        if (sums != nullptr) {
            if (sm[0]) atomicAdd(&sums[2 * b], (unsigned long long)sm[0]);
            if (sm[1]) atomicAdd(&sums[2 * b + 1], (unsigned long long)sm[1]);
        }
    }
    const size_t first = (size_t)row0 * W + col0;                                // 4. the runs
    en_store_run(out + (size_t)moff + first, n, [&](int j) { return (unsigned)pix[0][j]; });
    if (poff >= 0) en_store_run(out + (size_t)poff + first, n, [&](int j) { return (unsigned)pix[1][j]; });
    if (roff >= 0) en_store_run(out + (size_t)roff + first, n, [&](int j) { return (unsigned)pix[2][j]; });
    if (soff >= 0 && ooff >= 0) {
        const uint8_t* g = src + (size_t)soff + first;
        en_store_run(out + (size_t)ooff + 3 * first, 3 * n, [&](int j) {
            const int q = j / 3;
            const unsigned gray = g[q], p = pix[0][q];
            return (j - 3 * q == 1 && p > gray) ? p : gray;
        });
    }
}

const char* const EN_KIND[4] = {"mask", "overlay", "probability map", "spread map"};
struct Range {
    uintptr_t lo, hi;
    int image, kind;
};

}  // namespace

size_t uia_seg_native_ens_ws_bytes(int B) {
    if (B < 1 || B > EN_MAX_B) return 0;
    return ((size_t)B * EN_DESC * sizeof(int32_t) + 255) & ~(size_t)255;
}

int uia_seg_predict_native_ens_launch(hipStream_t stream, int K, int B, int S, const float* logits, uint32_t flips, float threshold, const uint8_t* src,
                                      size_t src_bytes, const int32_t* desc, uint8_t* out, size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats,
                                      uint64_t* sums) {
    const char* who = "uia_seg_predict_native_ens";
    UIA_CHECK_ARG(K >= 1 && K <= EN_MAX_K, "%s: K=%d members (1 <= K <= %d)", who, K, EN_MAX_K);
    UIA_CHECK_ARG(K == EN_MAX_K || (flips >> (2 * K)) == 0u, "%s: flips=0x%x has bits at or above 2 K = %d (two bits per member)", who, flips, 2 * K);
    UIA_CHECK_ARG(threshold > 0.0f && threshold < 1.0f, "%s: threshold %g (a finite value with 0 < threshold < 1)", who, (double)threshold);
    UIA_CHECK_ARG(B >= 1 && B <= EN_MAX_B && S >= EN_MIN_S && S <= EN_MAX_S, "%s: bad shape B=%d S=%d (1 <= B <= %d, %d <= S <= %d)", who, B, S, EN_MAX_B, EN_MIN_S,
                  EN_MAX_S);
    UIA_CHECK_ARG(logits && desc && out && ws && stats, "%s: null tensor (logits, desc, out, ws and stats are required)", who);
    UIA_CHECK_ARG(out_bytes >= 1 && out_bytes <= 0x7fffffffu, "%s: an output buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, out_bytes);
    UIA_CHECK_ARG(src == nullptr || (src_bytes >= 1 && src_bytes <= 0x7fffffffu), "%s: a source buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, src_bytes);
    UIA_CHECK_ARG((uintptr_t)logits % 4 == 0 && (uintptr_t)ws % 4 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)sums % 8 == 0,
                  "%s: logits, the workspace and stats must be 4-byte aligned, sums 8-byte aligned", who);
    UIA_CHECK_ARG(ws_bytes >= uia_seg_native_ens_ws_bytes(B), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, uia_seg_native_ens_ws_bytes(B));
    struct Fixed {
        uintptr_t lo, hi;
        const char* name;
    };
    const size_t member = (size_t)B * 2 * S * S;
    const Fixed fixed[5] = {{(uintptr_t)logits, (uintptr_t)logits + (size_t)K * member * sizeof(float), "logits"},
                            {(uintptr_t)src, (uintptr_t)src + (src ? src_bytes : 0), "src"},
                            {(uintptr_t)stats, (uintptr_t)stats + (size_t)B * EN_DESC * sizeof(int32_t), "stats"},
                            {(uintptr_t)sums, (uintptr_t)sums + (sums ? (size_t)B * 2 * sizeof(uint64_t) : 0), "sums"},
                            {(uintptr_t)ws, (uintptr_t)ws + uia_seg_native_ens_ws_bytes(B), "the workspace"}};
    for (int i = 0; i < 5; ++i)                                    // the inputs and the scratch among themselves: stats, sums and ws are written
        for (int j = (i < 2 ? 2 : i + 1); j < 5; ++j)
            UIA_CHECK_ARG(!(fixed[i].lo < fixed[j].hi && fixed[j].lo < fixed[i].hi), "%s: %s overlaps %s", who, fixed[i].name, fixed[j].name);
    std::vector<Range> ranges;
    ranges.reserve(4 * (size_t)B);
    unsigned tiles = 1;
    for (int b = 0; b < B; ++b) {                                  // every image is checked before anything is enqueued
        const int32_t* d = desc + (size_t)b * EN_DESC;
        const long long soff = d[0], H = d[1], W = d[2], moff = d[3], ooff = d[4], poff = d[5], roff = d[6];
        UIA_CHECK_ARG(d[7] == 0, "%s: image %d has a non-zero reserved descriptor word (%d)", who, b, d[7]);
        UIA_CHECK_ARG(H >= 1 && W >= 1 && H <= EN_MAX_SIDE && W <= EN_MAX_SIDE, "%s: image %d is %lld x %lld (1 .. %d a side)", who, b, H, W, EN_MAX_SIDE);
        UIA_CHECK_ARG(soff >= -1 && ooff >= -1 && poff >= -1 && roff >= -1,
                      "%s: image %d has source offset %lld, overlay offset %lld, probability offset %lld and spread offset %lld (an offset, or -1 for none)", who, b, soff,
                      ooff, poff, roff);
        const unsigned long long px = (unsigned long long)H * W;
        UIA_CHECK_ARG(moff >= 0 && (unsigned long long)moff + px <= out_bytes, "%s: the mask of image %d (offset %lld, %lld x %lld) leaves the output buffer of %zu bytes", who, b,
                      moff, H, W, out_bytes);
        ranges.push_back({(uintptr_t)out + (uintptr_t)moff, (uintptr_t)out + (uintptr_t)moff + (uintptr_t)px, b, 0});
        if (soff >= 0 && src != nullptr)                            // a source image is held to its buffer whether or not it is drawn
            UIA_CHECK_ARG((unsigned long long)soff + px <= src_bytes, "%s: image %d (offset %lld, %lld x %lld) leaves the source buffer of %zu bytes", who, b, soff, H, W,
                          src_bytes);
        if (soff >= 0 && ooff >= 0) {
            UIA_CHECK_ARG(src != nullptr, "%s: image %d asks for an overlay but src is null", who, b);
            UIA_CHECK_ARG((unsigned long long)ooff + 3 * px <= out_bytes, "%s: the overlay of image %d (offset %lld, %lld x %lld x 3) leaves the output buffer of %zu bytes",
                          who, b, ooff, H, W, out_bytes);
            ranges.push_back({(uintptr_t)out + (uintptr_t)ooff, (uintptr_t)out + (uintptr_t)ooff + (uintptr_t)(3 * px), b, 1});
        }
        const long long maps[2] = {poff, roff};
        for (int m = 0; m < 2; ++m)
            if (maps[m] >= 0) {
                UIA_CHECK_ARG((unsigned long long)maps[m] + px <= out_bytes, "%s: the %s of image %d (offset %lld, %lld x %lld) leaves the output buffer of %zu bytes", who,
                              EN_KIND[2 + m], b, maps[m], H, W, out_bytes);
                ranges.push_back({(uintptr_t)out + (uintptr_t)maps[m], (uintptr_t)out + (uintptr_t)maps[m] + (uintptr_t)px, b, 2 + m});
            }
        tiles = std::max(tiles, en_tiles(S, (int)H, (int)W));
    }
    for (const Range& r : ranges)
        for (int i = 0; i < 5; ++i)
            UIA_CHECK_ARG(!(r.lo < fixed[i].hi && fixed[i].lo < r.hi), "%s: the %s of image %d overlaps %s", who, EN_KIND[r.kind], r.image, fixed[i].name);
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.image < b.image; });
    for (size_t i = 1; i < ranges.size(); ++i)                     // sorted by start: two ranges overlap iff some neighbours do
        UIA_CHECK_ARG(ranges[i - 1].hi <= ranges[i].lo, "%s: the %s of image %d overlaps the %s of image %d", who, EN_KIND[ranges[i - 1].kind], ranges[i - 1].image,
                      EN_KIND[ranges[i].kind], ranges[i].image);

    UIA_CHECK_HIP(hipMemcpyAsync(ws, desc, (size_t)B * EN_DESC * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    const int words = B * EN_DESC;
    ens_init_kernel<<<dim3((unsigned)((words + EN_THREADS - 1) / EN_THREADS)), dim3(EN_THREADS), 0, stream>>>(words, stats, 2 * B, (unsigned long long*)sums);
    UIA_CHECK_LAUNCH();
    seg_native_ens_kernel<<<dim3(tiles, (unsigned)B), dim3(EN_THREADS), 0, stream>>>(K, S, flips, threshold, member, logits, src, out, (const int32_t*)ws, stats,
                                                                                   (unsigned long long*)sums);
    UIA_CHECK_LAUNCH();
    return 0;
}
