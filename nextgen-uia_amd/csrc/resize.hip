// resize.hip — uia_resize_batch: the `Image.resize` of the reference's loader workers (src/datasets/segmentation.py:171-202, classification.py:173-202; the
// contrastive loader's Resize + CenterCrop is the window form) on the device, for a batch of decoded images of different sizes, equal to Pillow 12.2 in
// every byte.  src/datasets/pil_resize.py is the same arithmetic in plain Python and the tests' oracle.
//
// Input: B images back to back in one byte buffer, 8 bits per channel, C in {1, 3} interleaved channels, at arbitrary byte offsets, and a HOST
// descriptor int32 [B][8]: (offset, H, W, mask offset or -1, dst_h, dst_w, y0, x0).  Image b is resampled to dst_h x dst_w and the S x S window at
// (y0, x0) of that result is written, planar, as (float)q / 255.0f; its mask (one byte per pixel, H x W) goes through Pillow's nearest scaler and is
// written as source byte != 0.  An image without a mask in a batch that has some gets a zero mask.
//
// uia_resize_batch_rgb is the same tile code for a batch that mixes gray and colour images (the contrastive loader: convert("RGB") when the mode is not
// RGB, Resize, CenterCrop): word 3 of the descriptor is the image's channel count, 1 or 3, there are no masks, the output has three planes, and a
// one-channel image is resampled once and written to all three — the channels of Pillow's convert("RGB") of an "L" image run the same arithmetic.
//
// Images: Pillow's two-pass 8-bit resample with the bicubic filter (a = -0.5), antialiased: per axis scale = in / dst, filterscale = max(scale, 1),
// support = 2 filterscale; output xx takes the source pixels xmin .. xmin + xmax - 1 around center = (xx + 0.5) scale with the weights
// bicubic((x + xmin - center + 0.5) / filterscale), summed in tap order and divided by the sum in float64, rounded to 22-bit fixed point; a pass is
// clip8((2^21 + sum pixel k) >> 22) in int32, columns first into an 8-bit intermediate, then rows.  An axis that keeps its size gets the one weight
// 2^22 on its own pixel, which is the copy Pillow makes by skipping that pass.  Masks: source index int(xo), xo = a / 2 stepped by a = in / dst in
// float64, the coordinate accumulated output by output (one thread per axis walks it from output 0).
//
// One workgroup of 256 threads makes a tile of TR rows x 32 columns of one image's window (all channels).  It computes its own coefficient tables in
// LDS (one thread per output column / row; the weights of a pixel are evaluated twice, once for the sum and once for the division, so no float64 table
// is kept), runs the horizontal pass over the source rows its TR output rows reach into an 8-bit intermediate IN LDS (36 KiB: rows x 32 x C bytes), and
// the vertical pass from there to the fp32 output: no workspace beyond the device copy of the descriptor, no second launch, nothing shared between
// workgroups.  TR (1 .. 16) is chosen on the host from the batch's largest vertical scale so that (TR - 1) scale + ksize rows fit the intermediate
// (ksize <= 129 is the contract's limit: a downscale of at most 32x); the kernel clamps the row count again.  Source pixels are read a byte at a time
// (any offset, any row pitch; neighbouring lanes read neighbouring bytes, served by L1); the output is written a float per lane, coalesced along the
// row.  Deterministic: no atomics.
#include <math.h>

#include "uia_common.h"
#include "uia_kernels.h"

namespace {

// see augment.hip: the product is handed through an empty asm statement so that nothing contracts it into the sum that follows
__device__ __forceinline__ double mul_rn(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

constexpr int RS_THREADS = 256;
constexpr int RS_TC = 32;                          // columns of a tile
constexpr int RS_TR_MAX = 16;                      // rows of a tile, at most
constexpr int RS_KMAX = 129;                       // taps per output pixel, at most
constexpr int RS_MID_BYTES = 36864;                // the 8-bit intermediate of a tile
constexpr int RS_MIN_S = 8, RS_MAX_S = 1024, RS_MAX_B = 65535, RS_MAX_DST = 16384;
constexpr int RS_DESC = 8;
constexpr int RS_BITS = 22;

__device__ __forceinline__ double rs_bicubic(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return __dadd_rn(mul_rn(mul_rn(__dadd_rn(mul_rn(1.5, x), -2.5), x), x), 1.0);
    if (x < 2.0) return mul_rn(__dadd_rn(mul_rn(__dadd_rn(mul_rn(__dadd_rn(x, -5.0), x), 8.0), x), -4.0), -0.5);
    return 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output xx of an axis n_in -> n_out: k[0 .. *cnt - 1], first source pixel *mn
__device__ void rs_coeffs(int n_in, int n_out, int xx, int* k, int* mn, int* cnt) {
    if (n_in == n_out) {                           // the pass Pillow skips
        k[0] = 1 << RS_BITS;
        *mn = xx;
        *cnt = 1;
        return;
    }
    const double scale = __ddiv_rn((double)n_in, (double)n_out);
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = mul_rn(2.0, fs);
    const double ss = __ddiv_rn(1.0, fs);
    const double center = mul_rn((double)xx + 0.5, scale);
    int xmin = (int)__dadd_rn(__dadd_rn(center, -support), 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)__dadd_rn(__dadd_rn(center, support), 0.5);
    if (xmax > n_in) xmax = n_in;
    const int n = min(max(xmax - xmin, 0), RS_KMAX);
    double ww = 0.0;
    for (int x = 0; x < n; ++x) ww = __dadd_rn(ww, rs_bicubic(mul_rn(__dadd_rn(__dadd_rn((double)(x + xmin), -center), 0.5), ss)));
    for (int x = 0; x < n; ++x) {
        double w = rs_bicubic(mul_rn(__dadd_rn(__dadd_rn((double)(x + xmin), -center), 0.5), ss));
        if (ww != 0.0) w = __ddiv_rn(w, ww);
        k[x] = w < 0.0 ? (int)__dadd_rn(-0.5, mul_rn(w, 4194304.0)) : (int)__dadd_rn(0.5, mul_rn(w, 4194304.0));
    }
    *mn = xmin;
    *cnt = n;
}

// Pillow's nearest scaler on one axis: idx[i] for outputs first .. first + count - 1, the coordinate accumulated from output 0
__device__ void rs_nearest(int n_in, int n_out, int first, int count, int* idx) {
    const double a = __ddiv_rn((double)n_in, (double)n_out);
    double xo = mul_rn(a, 0.5);
    for (int d = 0; d < first + count; ++d) {
        if (d >= first) idx[d - first] = min(max((int)xo, 0), n_in - 1);
        xo = __dadd_rn(xo, a);
    }
}

__device__ __forceinline__ int rs_clip8(int ss) { return min(max(ss >> RS_BITS, 0), 255); }

// The tile of one workgroup: C interleaved source channels, written to C planes, or (REPL, C = 1) the one plane written three times.  The LDS
// tables are the caller's, so that the two instantiations of the mixed kernel share them.
template <int C, bool REPL>
__device__ __forceinline__ void rs_tile(int S, int TR, const uint8_t* __restrict__ src, int off, int H, int W, int moff, int dst_h, int dst_w, int wy, int wx,
                                        float* __restrict__ out_images, uint8_t* __restrict__ out_masks, int (*hk)[RS_KMAX], int (*vk)[RS_KMAX], int* hmin,
                                        int* hcnt, int* vmin, int* vcnt, int* nx, int* ny, uint8_t* mid) {
    constexpr int PITCH = RS_TC * C;               // bytes of an intermediate row
    constexpr int ROWS_CAP = RS_MID_BYTES / PITCH;
    constexpr int OC = REPL ? 3 : C;               // planes of an output image

    const int tid = threadIdx.x;
    const size_t b = blockIdx.z;
    const int row0 = blockIdx.y * TR, col0 = blockIdx.x * RS_TC;                 // of the window
    const int TRh = min(min(TR, RS_TR_MAX), S - row0), TCw = min(RS_TC, S - col0);
    if (TRh <= 0 || TCw <= 0) return;
    const bool has_mask = out_masks != nullptr && moff >= 0;

    if (tid < TCw) rs_coeffs(W, dst_w, wx + col0 + tid, hk[tid], &hmin[tid], &hcnt[tid]);
    if (tid >= 64 && tid < 64 + TRh) rs_coeffs(H, dst_h, wy + row0 + tid - 64, vk[tid - 64], &vmin[tid - 64], &vcnt[tid - 64]);
    if (has_mask && tid == 128) rs_nearest(W, dst_w, wx + col0, TCw, nx);
    if (has_mask && tid == 192) rs_nearest(H, dst_h, wy + row0, TRh, ny);
    __syncthreads();

    // the source rows this tile's output rows reach: first pixels and ends both grow with the output index
    const int lo = vmin[0];
    const int R = min(min(vmin[TRh - 1] + vcnt[TRh - 1], H) - lo, ROWS_CAP);
    const uint8_t* img = src + (size_t)off;
    const int per_row = TCw * C;
    for (int i = tid; i < R * per_row; i += RS_THREADS) {                        // horizontal pass -> mid[r][x][c]
        const int r = i / per_row, rem = i - r * per_row;
        const int x = rem / C, c = rem - x * C;
        const uint8_t* p = img + ((size_t)(lo + r) * W + hmin[x]) * C + c;
        const int n = hcnt[x];
        int ss = 1 << (RS_BITS - 1);
        for (int k = 0; k < n; ++k) ss += (int)p[(size_t)k * C] * hk[x][k];
        mid[r * PITCH + rem] = (uint8_t)rs_clip8(ss);
    }
    __syncthreads();

    const int per_plane = TRh * TCw;
    for (int i = tid; i < C * per_plane; i += RS_THREADS) {                      // vertical pass -> fp32, planar
        const int c = i / per_plane, rem = i - c * per_plane;
        const int y = rem / TCw, x = rem - y * TCw;
        const int first = vmin[y] - lo;
        const int n = min(vcnt[y], R - first);                                  // (never smaller than vcnt[y] within the contract's limits)
        const uint8_t* p = mid + first * PITCH + x * C + c;
        int ss = 1 << (RS_BITS - 1);
        for (int k = 0; k < n; ++k) ss += (int)p[k * PITCH] * vk[y][k];
        const float v = (float)rs_clip8(ss) / 255.0f;
        float* o = out_images + ((b * OC + c) * S + (size_t)(row0 + y)) * S + col0 + x;
        o[0] = v;
        if (REPL) {                                                              // a gray image in a three-plane batch: convert("RGB") of "L" repeats the byte
            o[(size_t)S * S] = v;
            o[2 * (size_t)S * S] = v;
        }
    }

    if (out_masks != nullptr) {
        const uint8_t* msk = src + (size_t)max(moff, 0);
        for (int i = tid; i < per_plane; i += RS_THREADS) {
            const int y = i / TCw, x = i - y * TCw;
            const uint8_t v = has_mask ? (uint8_t)(msk[(size_t)ny[y] * W + nx[x]] != 0) : (uint8_t)0;
            out_masks[(b * S + (size_t)(row0 + y)) * S + col0 + x] = v;
        }
    }
}

#define RS_TILE_LDS                                                                                                     \
    __shared__ int hk[RS_TC][RS_KMAX], vk[RS_TR_MAX][RS_KMAX];                                                          \
    __shared__ int hmin[RS_TC], hcnt[RS_TC], vmin[RS_TR_MAX], vcnt[RS_TR_MAX], nx[RS_TC], ny[RS_TR_MAX];                \
    __shared__ uint8_t mid[RS_MID_BYTES]

template <int C>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(int S, int TR, const uint8_t* __restrict__ src, const int32_t* __restrict__ desc,
                                                            float* __restrict__ out_images, uint8_t* __restrict__ out_masks) {
    RS_TILE_LDS;
    const int32_t* d = desc + (size_t)blockIdx.z * RS_DESC;
    rs_tile<C, false>(S, TR, src, d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], out_images, out_masks, hk, vk, hmin, hcnt, vmin, vcnt, nx, ny, mid);
}

// uia_resize_batch_rgb: word 3 of the descriptor is the image's channel count; blockIdx.z is the image, so the branch is uniform over the workgroup
__global__ __launch_bounds__(RS_THREADS) void resize_rgb_kernel(int S, int TR, const uint8_t* __restrict__ src, const int32_t* __restrict__ desc,
                                                                float* __restrict__ out_images) {
    RS_TILE_LDS;
    const int32_t* d = desc + (size_t)blockIdx.z * RS_DESC;
    if (d[3] == 1)
        rs_tile<1, true>(S, TR, src, d[0], d[1], d[2], -1, d[4], d[5], d[6], d[7], out_images, nullptr, hk, vk, hmin, hcnt, vmin, vcnt, nx, ny, mid);
    else
        rs_tile<3, false>(S, TR, src, d[0], d[1], d[2], -1, d[4], d[5], d[6], d[7], out_images, nullptr, hk, vk, hmin, hcnt, vmin, vcnt, nx, ny, mid);
}

int rs_ksize(int n_in, int n_out) {
    const double scale = (double)n_in / (double)n_out;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

}  // namespace

size_t uia_resize_ws_bytes(int B) {
    if (B < 1 || B > RS_MAX_B) return 0;
    return ((size_t)B * RS_DESC * sizeof(int32_t) + 255) & ~(size_t)255;
}

// Both entries.  uia_resize_batch: C channels in and out, word 3 of an image is its mask offset.  uia_resize_batch_rgb (mixed): word 3 is the image's
// channel count, three planes out, no masks.
static int rs_launch(const char* who, bool mixed, hipStream_t stream, int B, int C, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws,
                     size_t ws_bytes, float* out_images, uint8_t* out_masks) {
    UIA_CHECK_ARG(B >= 1 && B <= RS_MAX_B && S >= RS_MIN_S && S <= RS_MAX_S, "%s: bad shape B=%d S=%d (1 <= B <= %d, %d <= S <= %d)", who, B, S, RS_MAX_B,
                  RS_MIN_S, RS_MAX_S);
    UIA_CHECK_ARG(C == 1 || C == 3, "%s: C=%d channels (1 or 3)", who, C);
    UIA_CHECK_ARG(src && desc && ws && out_images, "%s: null tensor", who);
    UIA_CHECK_ARG(src_bytes >= 1 && src_bytes <= 0x7fffffffu, "%s: a source buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, src_bytes);
    UIA_CHECK_ARG((uintptr_t)ws % 4 == 0 && (uintptr_t)out_images % 4 == 0, "%s: the workspace and out_images must be 4-byte aligned", who);
    UIA_CHECK_ARG(ws_bytes >= uia_resize_ws_bytes(B), "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, uia_resize_ws_bytes(B));
    const size_t pix = (size_t)S * S;
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; };
    UIA_CHECK_ARG(!overlap(src, src_bytes, out_images, (size_t)B * C * pix * sizeof(float)) && (!out_masks || !overlap(src, src_bytes, out_masks, (size_t)B * pix)) &&
                      (!out_masks || !overlap(out_images, (size_t)B * C * pix * sizeof(float), out_masks, (size_t)B * pix)),
                  "%s: the outputs must not be the inputs or each other (the ranges overlap)", who);
    int TR = RS_TR_MAX;
    for (int b = 0; b < B; ++b) {                                  // every image is checked before anything is enqueued
        const int32_t* d = desc + (size_t)b * RS_DESC;
        const long long off = d[0], H = d[1], W = d[2], moff = mixed ? -1 : d[3], dst_h = d[4], dst_w = d[5], y0 = d[6], x0 = d[7];
        const int Cb = mixed ? d[3] : C;
        UIA_CHECK_ARG(Cb == 1 || Cb == 3, "%s: image %d has %d channels (1 or 3)", who, b, Cb);
        UIA_CHECK_ARG(H >= 1 && W >= 1, "%s: image %d is %lld x %lld (H, W >= 1)", who, b, H, W);
        UIA_CHECK_ARG(off >= 0 && (unsigned long long)off + (unsigned long long)H * W * Cb <= src_bytes,
                      "%s: image %d (offset %lld, %lld x %lld x %d) leaves the source buffer of %zu bytes", who, b, off, H, W, Cb, src_bytes);
        UIA_CHECK_ARG(moff >= -1, "%s: image %d has mask offset %lld (an offset, or -1 for none)", who, b, moff);
        if (moff >= 0) {
            UIA_CHECK_ARG(out_masks != nullptr, "%s: image %d has a mask but out_masks is null", who, b);
            UIA_CHECK_ARG((unsigned long long)moff + (unsigned long long)H * W <= src_bytes, "%s: the mask of image %d (offset %lld, %lld x %lld) leaves the source buffer of %zu bytes",
                          who, b, moff, H, W, src_bytes);
        }
        UIA_CHECK_ARG(dst_h >= 1 && dst_w >= 1 && dst_h <= RS_MAX_DST && dst_w <= RS_MAX_DST, "%s: image %d is resampled to %lld x %lld (1 .. %d a side)", who, b,
                      dst_h, dst_w, RS_MAX_DST);
        UIA_CHECK_ARG(y0 >= 0 && x0 >= 0 && y0 + S <= dst_h && x0 + S <= dst_w, "%s: image %d: the %d x %d window at (%lld, %lld) leaves the %lld x %lld result", who, b,
                      S, S, y0, x0, dst_h, dst_w);
        const int kh = rs_ksize((int)W, (int)dst_w), kv = rs_ksize((int)H, (int)dst_h);
        UIA_CHECK_ARG(kh <= RS_KMAX && kv <= RS_KMAX, "%s: image %d: %lld x %lld -> %lld x %lld needs %d taps per pixel (at most %d: a downscale of at most 32x)", who,
                      b, H, W, dst_h, dst_w, kh > kv ? kh : kv, RS_KMAX);
        if (H != dst_h) {                                          // rows of a tile: (TR - 1) scale + ksize source rows must fit this image's intermediate
            const int rows_cap = RS_MID_BYTES / (RS_TC * Cb);
            const double scale = (double)H / (double)dst_h;
            const double fit = floor((double)(rows_cap - kv - 1) / scale) + 1.0;
            if (fit < (double)TR) TR = fit < 1.0 ? 1 : (int)fit;
        }
    }
    UIA_CHECK_HIP(hipMemcpyAsync(ws, desc, (size_t)B * RS_DESC * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    const dim3 grid((unsigned)((S + RS_TC - 1) / RS_TC), (unsigned)((S + TR - 1) / TR), (unsigned)B);
    if (mixed)
        resize_rgb_kernel<<<grid, dim3(RS_THREADS), 0, stream>>>(S, TR, src, (const int32_t*)ws, out_images);
    else if (C == 1)
        resize_kernel<1><<<grid, dim3(RS_THREADS), 0, stream>>>(S, TR, src, (const int32_t*)ws, out_images, out_masks);
    else
        resize_kernel<3><<<grid, dim3(RS_THREADS), 0, stream>>>(S, TR, src, (const int32_t*)ws, out_images, out_masks);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_resize_batch_launch(hipStream_t stream, int B, int C, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes,
                            float* out_images, uint8_t* out_masks) {
    return rs_launch("uia_resize_batch", false, stream, B, C, S, src, src_bytes, desc, ws, ws_bytes, out_images, out_masks);
}

int uia_resize_batch_rgb_launch(hipStream_t stream, int B, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes,
                                float* out_images) {
    return rs_launch("uia_resize_batch_rgb", true, stream, B, 3, S, src, src_bytes, desc, ws, ws_bytes, out_images, nullptr);
}

