// seg_viz.hip — the three pictures the segmentation test pass writes per image (reference src/utils/tools.py:278-315, visualize_seg), one launch per batch.
// Per pixel, from logits fp32 [B,2,S,S], channel 0 of images fp32 [B,Ci,S,S] and label [B,1,S,S] (uint8 or fp32):
//   g = (uint8)(x * 255)   one fp32 product, clamped to [0, 255] (NaN -> 0), truncated
//   t = label != 0 ? 255 : 0
//   p = argmax(logits) == 1 ? 255 : 0   torch's rules, the ones surface.hip and the Dice / IoU kernels use: a tie goes to class 0, NaN is the maximum
//   mask_rgb = (t, p, 0)      overlay_rgb = (max(g, t), max(g, p), g)      pred = p
// as plain row-major uint8 [B,S,S,3], [B,S,S,3] and [B,S,S]: the rows of three PNG files without their filter bytes.
// Pure streaming, 10 to 14 bytes in and 7 out per pixel, no LDS, no atomics, no scratch.  Two kernels:
//   quad_kernel    a thread owns four consecutive pixels of a row: 16-byte loads of the image and of both logit planes, 4 or 16 bytes of label, three dword
//                  stores per RGB output and one for pred.  Needs S % 4 == 0, the fp32 inputs on 16 bytes, uint8 labels and the outputs on 4.
//   pixel_kernel   a thread per pixel, byte stores: any S, fp32 inputs on 4 bytes, the rest on 1.
// uia_seg_viz_form says which of the two a call takes; it is a pure function of S, the label type and the addresses.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int SV_THREADS = 256;
constexpr int SV_MAXS = 16384;
constexpr unsigned long long SV_MAXPX = 1ull << 36;      // B * S * S (the grid is S * S / 256 or / 1024 blocks by min(B, 65535) rows of them)

__device__ __forceinline__ unsigned sv_grey(float x) {
    float v = __fmul_rn(x, 255.0f);                       // never contracted with anything: numpy's float32 product
    v = v > 0.0f ? v : 0.0f;                              // below 0 and NaN -> 0
    v = v < 255.0f ? v : 255.0f;
    return (unsigned)v;                                   // truncation, as astype(uint8) of an in-range value
}
// class 1 wins torch.argmax over (l0, l1): l0 is not NaN and (l1 is NaN or l1 > l0)
__device__ __forceinline__ unsigned sv_pred(float l0, float l1) { return (!(l0 != l0) && ((l1 != l1) || l1 > l0)) ? 255u : 0u; }
__device__ __forceinline__ unsigned sv_max(unsigned a, unsigned b) { return a > b ? a : b; }

// twelve bytes r0 g0 b0 r1 g1 b1 ... of four pixels as three little-endian dwords
__device__ __forceinline__ void sv_store_rgb4(unsigned char* dst, const unsigned (&r)[4], const unsigned (&g)[4], const unsigned (&b)[4]) {
    unsigned* d = (unsigned*)dst;
    d[0] = r[0] | (g[0] << 8) | (b[0] << 16) | (r[1] << 24);
    d[1] = g[1] | (b[1] << 8) | (r[2] << 16) | (g[2] << 24);
    d[2] = b[2] | (r[3] << 8) | (g[3] << 16) | (b[3] << 24);
}

template <bool LABEL_F32>
__device__ __forceinline__ void sv_quad(size_t b, size_t r, size_t plane, int Ci, const float* __restrict__ logits, const float* __restrict__ images,
                                        const void* __restrict__ labels, unsigned char* __restrict__ mask_rgb, unsigned char* __restrict__ overlay_rgb,
                                        unsigned char* __restrict__ pred) {
    const size_t px = b * plane + r;
    const f32x4 x = *(const f32x4*)(images + b * Ci * plane + r);
    const f32x4 l0 = *(const f32x4*)(logits + b * 2 * plane + r);
    const f32x4 l1 = *(const f32x4*)(logits + (b * 2 + 1) * plane + r);
    unsigned t[4], p[4], g[4], rr[4], gg[4], zero[4] = {0u, 0u, 0u, 0u};
    if (LABEL_F32) {
        const f32x4 lb = *(const f32x4*)((const float*)labels + px);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = lb[e] != 0.0f ? 255u : 0u;
    } else {
        const unsigned lb = *(const unsigned*)((const unsigned char*)labels + px);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = ((lb >> (8 * e)) & 0xFFu) ? 255u : 0u;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = sv_pred(l0[e], l1[e]);
        g[e] = sv_grey(x[e]);
        rr[e] = sv_max(g[e], t[e]);
        gg[e] = sv_max(g[e], p[e]);
    }
    sv_store_rgb4(mask_rgb + px * 3, t, p, zero);
    sv_store_rgb4(overlay_rgb + px * 3, rr, gg, g);
    *(unsigned*)(pred + px) = p[0] | (p[1] << 8) | (p[2] << 16) | (p[3] << 24);
}

template <bool LABEL_F32>
__global__ __launch_bounds__(SV_THREADS) void quad_kernel(int B, size_t plane, int Ci, const float* __restrict__ logits, const float* __restrict__ images,
                                                          const void* __restrict__ labels, unsigned char* __restrict__ mask_rgb,
                                                          unsigned char* __restrict__ overlay_rgb, unsigned char* __restrict__ pred) {
    const size_t r = ((size_t)blockIdx.x * SV_THREADS + threadIdx.x) * 4;      // S % 4 == 0: the four pixels lie in one row
    if (r >= plane) return;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) sv_quad<LABEL_F32>(b, r, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
}

template <bool LABEL_F32>
__device__ __forceinline__ void sv_pixel(size_t b, size_t r, size_t plane, int Ci, const float* __restrict__ logits, const float* __restrict__ images,
                                         const void* __restrict__ labels, unsigned char* __restrict__ mask_rgb, unsigned char* __restrict__ overlay_rgb,
                                         unsigned char* __restrict__ pred) {
    const size_t px = b * plane + r;
    const unsigned g = sv_grey(images[b * Ci * plane + r]);
    const unsigned p = sv_pred(logits[b * 2 * plane + r], logits[(b * 2 + 1) * plane + r]);
    const bool fg = LABEL_F32 ? ((const float*)labels)[px] != 0.0f : ((const unsigned char*)labels)[px] != 0;
    const unsigned t = fg ? 255u : 0u;
    unsigned char* m = mask_rgb + px * 3;
    unsigned char* o = overlay_rgb + px * 3;
    m[0] = (unsigned char)t;
    m[1] = (unsigned char)p;
    m[2] = 0;
    o[0] = (unsigned char)sv_max(g, t);
    o[1] = (unsigned char)sv_max(g, p);
    o[2] = (unsigned char)g;
    pred[px] = (unsigned char)p;
}

template <bool LABEL_F32>
__global__ __launch_bounds__(SV_THREADS) void pixel_kernel(int B, size_t plane, int Ci, const float* __restrict__ logits, const float* __restrict__ images,
                                                           const void* __restrict__ labels, unsigned char* __restrict__ mask_rgb,
                                                           unsigned char* __restrict__ overlay_rgb, unsigned char* __restrict__ pred) {
    const size_t r = (size_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (r >= plane) return;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) sv_pixel<LABEL_F32>(b, r, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
}

struct Span {
    uintptr_t lo, hi;
    const char* name;
};
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }
bool on(const void* p, unsigned n) { return ((uintptr_t)p % n) == 0; }

}  // namespace

int uia_seg_viz_form(int S, int label_dtype, const void* logits, const void* images, const void* labels, const void* mask_rgb, const void* overlay_rgb,
                     const void* pred) {
    if (S <= 0 || S % 4 != 0) return 0;
    if (!on(logits, 16) || !on(images, 16) || !on(labels, label_dtype == 1 ? 16 : 4)) return 0;
    return (on(mask_rgb, 4) && on(overlay_rgb, 4) && on(pred, 4)) ? 1 : 0;
}

int uia_seg_viz_launch(hipStream_t stream, int B, int C, int Ci, int S, const float* logits, const float* images, const void* labels, int label_dtype,
                       uint8_t* mask_rgb, uint8_t* overlay_rgb, uint8_t* pred) {
    UIA_CHECK_ARG(logits && images && labels && mask_rgb && overlay_rgb && pred, "uia_seg_viz: null tensor");
    UIA_CHECK_ARG(B >= 1 && S >= 1 && S <= SV_MAXS, "uia_seg_viz: bad shape B=%d S=%d (B >= 1, 1 <= S <= %d)", B, S, SV_MAXS);
    UIA_CHECK_ARG(C == 2, "uia_seg_viz: %d classes (binary masks only: 2)", C);
    UIA_CHECK_ARG(Ci == 1 || Ci == 3, "uia_seg_viz: %d image channels (1 or 3)", Ci);
    UIA_CHECK_ARG(label_dtype == 0 || label_dtype == 1, "uia_seg_viz: unknown label dtype code %d (0: uint8, 1: fp32)", label_dtype);
    const size_t plane = (size_t)S * S, total = (size_t)B * plane;
    UIA_CHECK_ARG(total <= SV_MAXPX, "uia_seg_viz: %zu pixels in the batch (at most %llu)", total, SV_MAXPX);
    UIA_CHECK_ARG(on(logits, 4) && on(images, 4) && (label_dtype == 0 || on(labels, 4)), "uia_seg_viz: an fp32 input is not on a 4-byte address");
    const Span spans[6] = {{(uintptr_t)mask_rgb, (uintptr_t)mask_rgb + total * 3, "mask_rgb"},
                           {(uintptr_t)overlay_rgb, (uintptr_t)overlay_rgb + total * 3, "overlay_rgb"},
                           {(uintptr_t)pred, (uintptr_t)pred + total, "pred"},
                           {(uintptr_t)logits, (uintptr_t)logits + total * 2 * sizeof(float), "logits"},
                           {(uintptr_t)images, (uintptr_t)images + total * Ci * sizeof(float), "images"},
                           {(uintptr_t)labels, (uintptr_t)labels + total * (label_dtype == 1 ? sizeof(float) : 1), "labels"}};
    for (int i = 0; i < 3; ++i)                            // an output against every later output and every input
        for (int j = i + 1; j < 6; ++j) UIA_CHECK_ARG(!overlap(spans[i], spans[j]), "uia_seg_viz: %s overlaps %s", spans[i].name, spans[j].name);
    const bool quad = uia_seg_viz_form(S, label_dtype, logits, images, labels, mask_rgb, overlay_rgb, pred) == 1;
    const size_t work = quad ? plane / 4 : plane;          // threads per image; blockIdx.y walks the images: no division in the kernels
    const dim3 grid((unsigned)((work + SV_THREADS - 1) / SV_THREADS), (unsigned)(B < 65535 ? B : 65535)), block(SV_THREADS);
    if (quad) {
        if (label_dtype == 1)
            hipLaunchKernelGGL(quad_kernel<true>, grid, block, 0, stream, B, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
        else
            hipLaunchKernelGGL(quad_kernel<false>, grid, block, 0, stream, B, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
    } else {
        if (label_dtype == 1)
            hipLaunchKernelGGL(pixel_kernel<true>, grid, block, 0, stream, B, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
        else
            hipLaunchKernelGGL(pixel_kernel<false>, grid, block, 0, stream, B, plane, Ci, logits, images, labels, mask_rgb, overlay_rgb, pred);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}
