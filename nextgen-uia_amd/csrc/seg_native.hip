// seg_native.hip — uia_seg_predict_native: the way back from a model's S x S logits to each image's own H x W, one launch per batch.  The inverse of
// uia_resize_batch's square squash (resize.hip), under its conventions and uia_seg_viz's (seg_viz.hip): the batch's ragged DEVICE byte buffer as the
// prefetcher copied it, a HOST descriptor int32 [B][8] copied to the workspace on the stream, everything checked before anything is enqueued.
//
// Per image b, descriptor (src_offset or -1, H, W, mask_out_offset, overlay_out_offset or -1, 0, 0, 0), and native pixel (y, x), the two planes of
// logits fp32 [B,2,S,S] are sampled as torch.nn.functional.interpolate(size=(H, W), mode="bilinear", align_corners=False) samples them, in fp32, every
// product and sum rounded once (nothing is contracted into an fma):
//   scale_y = (float)S / (float)H        sy = max(scale_y * ((float)y + 0.5f) - 0.5f, 0)       y0 = (int)sy   y1 = min(y0 + 1, S - 1)   ly = sy - y0
//   the same for x;  the four taps are combined rows first, then columns, per plane c:
//   v_c[k] = (1 - ly) * L_c[y0][k] + ly * L_c[y1][k]      (k = x0, x1)          u_c = (1 - lx) * v_c[x0] + lx * v_c[x1]
//   A tap whose weight is exactly 0 does not enter: ly == 0 gives v_c[k] = L_c[y0][k], lx == 0 gives u_c = v_c[x0].  At H = W = S every ly and lx is 0 and
//   u_c is the logit itself, infinities and NaN included.
//   p = 255 where argmax over (u_0, u_1) is class 1 by torch's rules (a tie, -0.0 against +0.0 included, goes to class 0; NaN is the maximum; NaN in
//   both goes to class 0), the rule of uia_seg_viz, else 0.
// Outputs, inside the one byte buffer `out`: the mask, H * W bytes of p at mask_out_offset, plain row-major; when src_offset and overlay_out_offset
// are both >= 0 the overlay, H * W * 3 bytes (g, max(g, p), g) at overlay_out_offset with g the source byte at src_offset + y * W + x; and
// stats[b] = (foreground pixels, ymin, xmin, ymax, xmax, 0, 0, 0), which a small launch ahead of the kernel sets to (0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0).
//
// One workgroup of 256 threads makes TR whole rows of one image (grid: row tile x image), TR = sn_rows(S, W) between 1 and 8 so that the rows' bytes fit
// the LDS below.  Whole rows of a row-major image are one contiguous run of n = rows * W pixels in the mask, 3 n bytes in the overlay and n in the source.
//   1. the rows' vertical blends of both planes, (v_0, v_1) pairs [TR][S], into LDS (32 KiB): coalesced reads of the 2 x 2 logit rows a native row needs;
//   2. a thread per pixel: two 8-byte LDS reads, the horizontal blend, p into a byte of LDS (16 KiB); the pixel's part of the statistics stays in
//      registers, is folded with LDS integer atomics per thread and with five global integer atomics per workgroup that saw foreground;
//   3. the runs are written from LDS.  Offsets are arbitrary bytes, so nothing is assumed about an address: each run is walked in the ALIGNED dwords that
//      cover it, decided per run inside the kernel: a dword wholly inside the run is one 4-byte store, the ragged first and last ones are byte stores.
// Source bytes are read a byte at a time (any offset; neighbouring lanes read neighbouring bytes).  Deterministic: integer atomics only.
#include <limits.h>

#include <algorithm>
#include <vector>

#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int SN_THREADS = 256;
constexpr int SN_MIN_S = 8, SN_MAX_S = 1024, SN_MAX_B = 65535, SN_MAX_SIDE = 16384;
constexpr int SN_DESC = 8;
constexpr int SN_TR_MAX = 8;                       // rows of a tile, at most
constexpr int SN_BLEND = 4096;                     // (v_0, v_1) pairs of a tile's vertical blends: TR * S of them
constexpr int SN_PIX = 16384;                      // predicted bytes of a tile: TR * W of them

// rows of a tile of an image W wide under logits S x S: the same on the host (the grid) and in the kernel
__host__ __device__ inline int sn_rows(int S, int W) {
    int tr = SN_BLEND / S < SN_PIX / W ? SN_BLEND / S : SN_PIX / W;
    tr = tr < SN_TR_MAX ? tr : SN_TR_MAX;
    return tr < 1 ? 1 : tr;
}

// a product nothing can contract into the sum that follows (see augment.hip): handed through an empty asm statement
__device__ __forceinline__ float sn_mul(float a, float b) {
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// source coordinate of output index i: area_pixel_compute_source_index of torch's upsample kernels (align_corners = False, not cubic)
__device__ __forceinline__ void sn_coord(float scale, int i, int S, int& i0, int& i1, float& l) {
    float s = sn_mul(scale, (float)i + 0.5f) - 0.5f;
    s = s > 0.0f ? s : 0.0f;
    i0 = min((int)s, S - 1);
    i1 = min(i0 + 1, S - 1);
    l = s - (float)i0;
}
__device__ __forceinline__ float sn_blend(float a, float b, float l) {
    return l == 0.0f ? a : sn_mul(1.0f - l, a) + sn_mul(l, b);
}
// class 1 wins torch.argmax over (u0, u1): u0 is not NaN and (u1 is NaN or u1 > u0) — seg_viz.hip's sv_pred
__device__ __forceinline__ unsigned sn_pred(float u0, float u1) { return (!(u0 != u0) && ((u1 != u1) || u1 > u0)) ? 255u : 0u; }

// Writes bytes f(0) .. f(n - 1) to dst .. dst + n - 1: the aligned dwords that cover the run are shared out over the workgroup
template <typename F>
__device__ __forceinline__ void sn_store_run(uint8_t* dst, int n, F f) {
    const int a = (int)((uintptr_t)dst & 3u);      // the run starts `a` bytes into its first dword
    const int words = (n + a + 3) >> 2;
    for (int k = threadIdx.x; k < words; k += SN_THREADS) {
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

__global__ __launch_bounds__(SN_THREADS) void stats_init_kernel(int n, int32_t* __restrict__ stats) {
    const int i = blockIdx.x * SN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int w = i & (SN_DESC - 1);
    stats[i] = (w == 1 || w == 2) ? INT_MAX : ((w == 3 || w == 4) ? -1 : 0);
}

__global__ __launch_bounds__(SN_THREADS) void seg_native_kernel(int S, const float* __restrict__ logits, const uint8_t* __restrict__ src,
                                                                uint8_t* __restrict__ out, const int32_t* __restrict__ desc, int32_t* __restrict__ stats) {
    __shared__ float2 blend[SN_BLEND];
    __shared__ uint8_t pix[SN_PIX];
    __shared__ int st[5];

    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int32_t* d = desc + b * SN_DESC;
    const int soff = d[0], H = d[1], W = d[2], moff = d[3], ooff = d[4];
    const int TR = sn_rows(S, W);
    const int row0 = blockIdx.x * TR;
    if (row0 >= H) return;                         // (uniform over the workgroup: nobody waits at a barrier below)
    const int rows = min(TR, H - row0);
    const int n = rows * W;                        // <= SN_PIX
    const float scale_y = __fdiv_rn((float)S, (float)H), scale_x = __fdiv_rn((float)S, (float)W);      // IEEE division, not a reciprocal
    const float* L0 = logits + b * 2 * (size_t)S * S;
    const float* L1 = L0 + (size_t)S * S;

    if (tid == 0) {
        st[0] = 0;
        st[1] = st[2] = INT_MAX;
        st[3] = st[4] = -1;
    }
    for (int i = tid; i < rows * S; i += SN_THREADS) {                           // 1. vertical blends
        const int r = i / S, k = i - r * S;
        int y0, y1;
        float ly;
        sn_coord(scale_y, row0 + r, S, y0, y1, ly);
        float2 v;
        v.x = sn_blend(L0[(size_t)y0 * S + k], L0[(size_t)y1 * S + k], ly);
        v.y = sn_blend(L1[(size_t)y0 * S + k], L1[(size_t)y1 * S + k], ly);
        blend[i] = v;
    }
    __syncthreads();

    int cnt = 0, ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1;
    for (int i = tid; i < n; i += SN_THREADS) {                                  // 2. horizontal blends, the prediction, the statistics
        const int r = i / W, x = i - r * W;
        int x0, x1;
        float lx;
        sn_coord(scale_x, x, S, x0, x1, lx);
        const float2 va = blend[r * S + x0], vb = blend[r * S + x1];
        const unsigned p = sn_pred(sn_blend(va.x, vb.x, lx), sn_blend(va.y, vb.y, lx));
        pix[i] = (uint8_t)p;
        if (p) {
            const int y = row0 + r;
            ++cnt;
            ymin = min(ymin, y);
            ymax = max(ymax, y);
            xmin = min(xmin, x);
            xmax = max(xmax, x);
        }
    }
    if (cnt) {
        atomicAdd(&st[0], cnt);
        atomicMin(&st[1], ymin);
        atomicMin(&st[2], xmin);
        atomicMax(&st[3], ymax);
        atomicMax(&st[4], xmax);
    }
    __syncthreads();

    if (tid == 0 && st[0]) {
        int32_t* s = stats + b * SN_DESC;
        atomicAdd(&s[0], st[0]);
        atomicMin(&s[1], st[1]);
        atomicMin(&s[2], st[2]);
        atomicMax(&s[3], st[3]);
        atomicMax(&s[4], st[4]);
    }
    const size_t first = (size_t)row0 * W;                                       // 3. the runs
    sn_store_run(out + (size_t)moff + first, n, [&](int j) { return (unsigned)pix[j]; });
    if (soff >= 0 && ooff >= 0) {
        const uint8_t* g = src + (size_t)soff + first;
        sn_store_run(out + (size_t)ooff + 3 * first, 3 * n, [&](int j) {
            const int q = j / 3;
            const unsigned gray = g[q], p = pix[q];
            return (j - 3 * q == 1 && p > gray) ? p : gray;
        });
    }
}

struct Range {
    uintptr_t lo, hi;
    int image;
    bool overlay;
};

}  // namespace

size_t uia_seg_native_ws_bytes(int B) {
    if (B < 1 || B > SN_MAX_B) return 0;
    return ((size_t)B * SN_DESC * sizeof(int32_t) + 255) & ~(size_t)255;
}

int uia_seg_predict_native_launch(hipStream_t stream, int B, int S, const float* logits, const uint8_t* src, size_t src_bytes, const int32_t* desc, uint8_t* out,
                                  size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats) {
    const char* who = "uia_seg_predict_native";
    UIA_CHECK_ARG(B >= 1 && B <= SN_MAX_B && S >= SN_MIN_S && S <= SN_MAX_S, "%s: bad shape B=%d S=%d (1 <= B <= %d, %d <= S <= %d)", who, B, S, SN_MAX_B, SN_MIN_S,
                  SN_MAX_S);
    UIA_CHECK_ARG(logits && desc && out && ws && stats, "%s: null tensor (logits, desc, out, ws and stats are required)", who);
    UIA_CHECK_ARG(out_bytes >= 1 && out_bytes <= 0x7fffffffu, "%s: an output buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, out_bytes);
    UIA_CHECK_ARG(src == nullptr || (src_bytes >= 1 && src_bytes <= 0x7fffffffu), "%s: a source buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, src_bytes);
    UIA_CHECK_ARG((uintptr_t)logits % 4 == 0 && (uintptr_t)ws % 4 == 0 && (uintptr_t)stats % 4 == 0, "%s: logits, the workspace and stats must be 4-byte aligned", who);
    UIA_CHECK_ARG(ws_bytes >= uia_seg_native_ws_bytes(B), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, uia_seg_native_ws_bytes(B));
    struct Fixed {
        uintptr_t lo, hi;
        const char* name;
    };
    const Fixed fixed[4] = {{(uintptr_t)logits, (uintptr_t)logits + (size_t)B * 2 * S * S * sizeof(float), "logits"},
                            {(uintptr_t)src, (uintptr_t)src + (src ? src_bytes : 0), "src"},
                            {(uintptr_t)stats, (uintptr_t)stats + (size_t)B * SN_DESC * sizeof(int32_t), "stats"},
                            {(uintptr_t)ws, (uintptr_t)ws + uia_seg_native_ws_bytes(B), "the workspace"}};
    for (int i = 0; i < 4; ++i)                                    // the inputs and the scratch among themselves: stats and ws are written
        for (int j = (i < 2 ? 2 : i + 1); j < 4; ++j)
            UIA_CHECK_ARG(!(fixed[i].lo < fixed[j].hi && fixed[j].lo < fixed[i].hi), "%s: %s overlaps %s", who, fixed[i].name, fixed[j].name);
    std::vector<Range> ranges;
    ranges.reserve(2 * (size_t)B);
    unsigned tiles = 1;
    for (int b = 0; b < B; ++b) {                                  // every image is checked before anything is enqueued
        const int32_t* d = desc + (size_t)b * SN_DESC;
        const long long soff = d[0], H = d[1], W = d[2], moff = d[3], ooff = d[4];
        UIA_CHECK_ARG(d[5] == 0 && d[6] == 0 && d[7] == 0, "%s: image %d has a non-zero reserved descriptor word (%d, %d, %d)", who, b, d[5], d[6], d[7]);
        UIA_CHECK_ARG(H >= 1 && W >= 1 && H <= SN_MAX_SIDE && W <= SN_MAX_SIDE, "%s: image %d is %lld x %lld (1 .. %d a side)", who, b, H, W, SN_MAX_SIDE);
        UIA_CHECK_ARG(soff >= -1 && ooff >= -1, "%s: image %d has source offset %lld and overlay offset %lld (an offset, or -1 for none)", who, b, soff, ooff);
        const unsigned long long px = (unsigned long long)H * W;
        UIA_CHECK_ARG(moff >= 0 && (unsigned long long)moff + px <= out_bytes, "%s: the mask of image %d (offset %lld, %lld x %lld) leaves the output buffer of %zu bytes", who, b,
                      moff, H, W, out_bytes);
        ranges.push_back({(uintptr_t)out + (uintptr_t)moff, (uintptr_t)out + (uintptr_t)moff + (uintptr_t)px, b, false});
        if (soff >= 0 && src != nullptr)                            // a source image is held to its buffer whether or not it is drawn
            UIA_CHECK_ARG((unsigned long long)soff + px <= src_bytes, "%s: image %d (offset %lld, %lld x %lld) leaves the source buffer of %zu bytes", who, b, soff, H, W,
                          src_bytes);
        if (soff >= 0 && ooff >= 0) {
            UIA_CHECK_ARG(src != nullptr, "%s: image %d asks for an overlay but src is null", who, b);
            UIA_CHECK_ARG((unsigned long long)ooff + 3 * px <= out_bytes, "%s: the overlay of image %d (offset %lld, %lld x %lld x 3) leaves the output buffer of %zu bytes",
                          who, b, ooff, H, W, out_bytes);
            ranges.push_back({(uintptr_t)out + (uintptr_t)ooff, (uintptr_t)out + (uintptr_t)ooff + (uintptr_t)(3 * px), b, true});
        }
        const int tr = sn_rows(S, (int)W);
        tiles = std::max(tiles, (unsigned)((H + tr - 1) / tr));
    }
    for (const Range& r : ranges)
        for (int i = 0; i < 4; ++i)
            UIA_CHECK_ARG(!(r.lo < fixed[i].hi && fixed[i].lo < r.hi), "%s: the %s of image %d overlaps %s", who, r.overlay ? "overlay" : "mask", r.image, fixed[i].name);
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.image < b.image; });
    for (size_t i = 1; i < ranges.size(); ++i)                     // sorted by start: two ranges overlap iff some neighbours do
        UIA_CHECK_ARG(ranges[i - 1].hi <= ranges[i].lo, "%s: the %s of image %d overlaps the %s of image %d", who, ranges[i - 1].overlay ? "overlay" : "mask",
                      ranges[i - 1].image, ranges[i].overlay ? "overlay" : "mask", ranges[i].image);

    UIA_CHECK_HIP(hipMemcpyAsync(ws, desc, (size_t)B * SN_DESC * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    const int words = B * SN_DESC;
    stats_init_kernel<<<dim3((unsigned)((words + SN_THREADS - 1) / SN_THREADS)), dim3(SN_THREADS), 0, stream>>>(words, stats);
    UIA_CHECK_LAUNCH();
    seg_native_kernel<<<dim3(tiles, (unsigned)B), dim3(SN_THREADS), 0, stream>>>(S, logits, src, out, (const int32_t*)ws, stats);
    UIA_CHECK_LAUNCH();
    return 0;
}
