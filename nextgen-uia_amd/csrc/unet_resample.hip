// unet_resample.hip — the two resampling ops of the DINOv2 UNet decoder, forward and backward, both in gather form (no atomics; every
// output element sums its taps in a fixed order, so runs are bit-identical).
//
// uia_upsample_ac: nn.Upsample(scale_factor=f, mode="bilinear", align_corners=True) on NHWC [B, H, W, C] -> [B, fH, fW, C]
//   (UNetDecoderUpBlock.forward, the reference's src/third_party/dino/dinov2.py:146-152).  Source index of output o: o·(H−1)/(fH−1),
//   as ATen computes it for align_corners.  The backward walks, for each source pixel, the output rows / columns whose two taps can
//   reach it and adds their weights in output order.
// uia_resize_aa: F.interpolate(size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False), what torchvision's
//   transforms.Resize(BICUBIC) runs on a float tensor (UNetDecoder.forward's resize_image).  Separable: a horizontal pass of the NHWC input
//   into an fp32 [B, C, Hi, Wo] scratch, then a vertical pass into the NCHW fp32 [B, C, Ho, Wo] logits; the backward runs the two
//   passes' transposes in gather form.  Weights as ATen's _upsample_bicubic2d_aa: scale = in/out, support = 2·max(scale, 1), cubic
//   a = −0.5 evaluated at (j − centre + 0.5)/max(scale, 1), normalised per output index.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

// ---------------------------------------------------------------- bilinear, align_corners = True
struct Lin {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Lin lin_taps(int o, int in, float scale) {
    const float src = scale * (float)o;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    const int i1 = i0 < in - 1 ? i0 + 1 : i0;
    const float l1 = src - (float)i0;
    return Lin{i0, i1, 1.f - l1, l1};
}
__device__ __forceinline__ float lin_weight(int o, int i, int in, float scale) {
    const Lin t = lin_taps(o, in, scale);
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void upsample_ac_fwd_kernel(int B, int H, int W, int C, int f, float sy, float sx, const T* __restrict__ in,
                                                              T* __restrict__ out) {
    const int Ho = H * f, Wo = W * f;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Ho * Wo * C) return;
    const int c = (int)(i % C);
    const long p = i / C;
    const int x = (int)(p % Wo), y = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
    const Lin ty = lin_taps(y, H, sy), tx = lin_taps(x, W, sx);
    const T* base = in + (long)b * H * W * C + c;
    const float v00 = to_f32(base[((long)ty.i0 * W + tx.i0) * C]), v01 = to_f32(base[((long)ty.i0 * W + tx.i1) * C]);
    const float v10 = to_f32(base[((long)ty.i1 * W + tx.i0) * C]), v11 = to_f32(base[((long)ty.i1 * W + tx.i1) * C]);
    out[i] = from_f32<T>(ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11));
}

// outputs o of an axis whose taps can touch source index i: src(o) within (i − 1, i + 1)
__device__ __forceinline__ void lin_range(int i, int in, int out, float scale, int& lo, int& hi) {
    if (in == 1 || scale == 0.f) { lo = 0; hi = out - 1; return; }
    lo = (int)floorf((float)(i - 1) / scale) - 1;
    hi = (int)ceilf((float)(i + 1) / scale) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > out - 1 ? out - 1 : hi;
}

template <typename T>
__global__ __launch_bounds__(256) void upsample_ac_bwd_kernel(int B, int H, int W, int C, int f, float sy, float sx, const T* __restrict__ dout,
                                                              T* __restrict__ din) {
    const int Ho = H * f, Wo = W * f;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H * W * C) return;
    const int c = (int)(i % C);
    const long p = i / C;
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((long)W * H));
    int ylo, yhi, xlo, xhi;
    lin_range(y, H, Ho, sy, ylo, yhi);
    lin_range(x, W, Wo, sx, xlo, xhi);
    const T* base = dout + (long)b * Ho * Wo * C + c;
    float s = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = lin_weight(oy, y, H, sy);
        if (wy == 0.f) continue;
        float r = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = lin_weight(ox, x, W, sx);
            if (wx != 0.f) r = fmaf(wx, to_f32(base[((long)oy * Wo + ox) * C]), r);
        }
        s = fmaf(wy, r, s);
    }
    din[i] = from_f32<T>(s);
}

// ---------------------------------------------------------------- antialiased bicubic
constexpr int AA_MAX_TAPS = 16;

__device__ __forceinline__ float aa_cubic(float x) {
    const float a = -0.5f;
    x = fabsf(x);
    if (x < 1.f) return ((a + 2.f) * x - (a + 3.f)) * x * x + 1.f;
    if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * a;
    return 0.f;
}
// window [xmin, xmin + n) of output index i and its normalised weights
__device__ __forceinline__ int aa_window(int i, int in, float scale, float (&w)[AA_MAX_TAPS], int& xmin) {
    const float support = scale >= 1.f ? 2.f * scale : 2.f;
    const float invscale = scale >= 1.f ? 1.f / scale : 1.f;
    const float center = scale * ((float)i + 0.5f);
    int lo = (int)(center - support + 0.5f);
    lo = lo < 0 ? 0 : lo;
    int hi = (int)(center + support + 0.5f);
    hi = hi > in ? in : hi;
    int n = hi - lo;
    n = n > AA_MAX_TAPS ? AA_MAX_TAPS : n;
    float total = 0.f;
    for (int j = 0; j < n; ++j) {
        w[j] = aa_cubic(((float)(j + lo) - center + 0.5f) * invscale);
        total += w[j];
    }
    const float inv = total != 0.f ? 1.f / total : 0.f;
    for (int j = 0; j < n; ++j) w[j] *= inv;
    xmin = lo;
    return n;
}
// weight of source index j in the window of output index i (0 outside)
__device__ __forceinline__ float aa_weight(int i, int j, int in, float scale) {
    float w[AA_MAX_TAPS];
    int lo;
    const int n = aa_window(i, in, scale, w, lo);
    float r = 0.f;
    for (int k = 0; k < n; ++k)
        if (lo + k == j) r = w[k];
    return r;
}
// output indices whose window can hold source index j
__device__ __forceinline__ void aa_range(int j, int in, int out, float scale, int& lo, int& hi) {
    const float support = scale >= 1.f ? 2.f * scale : 2.f;
    lo = (int)floorf(((float)j - support) / scale - 0.5f) - 1;
    hi = (int)ceilf(((float)j + 1.f + support) / scale - 0.5f) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > out - 1 ? out - 1 : hi;
}

// horizontal pass: x NHWC [B, Hi, Wi, C] -> tmp [B, C, Hi, Wo]
template <typename T>
__global__ __launch_bounds__(256) void aa_h_fwd_kernel(int B, int C, int Hi, int Wi, int Wo, float scale, const T* __restrict__ x, float* __restrict__ tmp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C * Hi * Wo) return;
    const int ox = (int)(i % Wo), y = (int)((i / Wo) % Hi), c = (int)((i / ((long)Wo * Hi)) % C), b = (int)(i / ((long)Wo * Hi * C));
    float w[AA_MAX_TAPS];
    int lo;
    const int n = aa_window(ox, Wi, scale, w, lo);
    const T* row = x + (((long)b * Hi + y) * Wi) * C + c;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(w[k], to_f32(row[(long)(lo + k) * C]), s);
    tmp[i] = s;
}
// vertical pass: tmp [B, C, Hi, Wo] -> out [B, C, Ho, Wo]
__global__ __launch_bounds__(256) void aa_v_fwd_kernel(long planes, int Hi, int Ho, int Wo, float scale, const float* __restrict__ tmp, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * Ho * Wo) return;
    const int x = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const long pl = i / ((long)Wo * Ho);
    float w[AA_MAX_TAPS];
    int lo;
    const int n = aa_window(oy, Hi, scale, w, lo);
    const float* col = tmp + pl * Hi * Wo + x;
    float s = 0.f;
    for (int k = 0; k < n; ++k) s = fmaf(w[k], col[(long)(lo + k) * Wo], s);
    out[i] = s;
}
// vertical transpose: dout [B, C, Ho, Wo] -> dtmp [B, C, Hi, Wo]
__global__ __launch_bounds__(256) void aa_v_bwd_kernel(long planes, int Hi, int Ho, int Wo, float scale, const float* __restrict__ dout, float* __restrict__ dtmp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * Hi * Wo) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Hi);
    const long pl = i / ((long)Wo * Hi);
    int lo, hi;
    aa_range(y, Hi, Ho, scale, lo, hi);
    const float* col = dout + pl * Ho * Wo + x;
    float s = 0.f;
    for (int oy = lo; oy <= hi; ++oy) {
        const float w = aa_weight(oy, y, Hi, scale);
        if (w != 0.f) s = fmaf(w, col[(long)oy * Wo], s);
    }
    dtmp[i] = s;
}
// horizontal transpose: dtmp [B, C, Hi, Wo] -> dx NHWC [B, Hi, Wi, C]
template <typename T>
__global__ __launch_bounds__(256) void aa_h_bwd_kernel(int B, int C, int Hi, int Wi, int Wo, float scale, const float* __restrict__ dtmp, T* __restrict__ dx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Hi * Wi * C) return;
    const int c = (int)(i % C), x = (int)((i / C) % Wi), y = (int)((i / ((long)C * Wi)) % Hi), b = (int)(i / ((long)C * Wi * Hi));
    int lo, hi;
    aa_range(x, Wi, Wo, scale, lo, hi);
    const float* row = dtmp + (((long)b * C + c) * Hi + y) * Wo;
    float s = 0.f;
    for (int ox = lo; ox <= hi; ++ox) {
        const float w = aa_weight(ox, x, Wi, scale);
        if (w != 0.f) s = fmaf(w, row[ox], s);
    }
    dx[i] = from_f32<T>(s);
}

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int uia_upsample_ac_launch(hipStream_t stream, int dtype, int backward, int B, int H, int W, int C, int f, const void* in, void* out) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_upsample_ac: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && f >= 1 && f <= 64, "uia_upsample_ac: B=%d H=%d W=%d C=%d f=%d out of range", B, H, W, C, f);
    UIA_CHECK_ARG((long)B * H * W * C * f * f < (1l << 40), "uia_upsample_ac: shape too large");
    UIA_CHECK_ARG(in && out, "uia_upsample_ac: null tensor");
    const int Ho = H * f, Wo = W * f;
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    if (!backward) {
        const long n = (long)B * Ho * Wo * C;
        if (dtype == UIA_BF16) hipLaunchKernelGGL(upsample_ac_fwd_kernel<bf16_t>, dim3(blocks(n)), dim3(256), 0, stream, B, H, W, C, f, sy, sx, (const bf16_t*)in, (bf16_t*)out);
        else hipLaunchKernelGGL(upsample_ac_fwd_kernel<float>, dim3(blocks(n)), dim3(256), 0, stream, B, H, W, C, f, sy, sx, (const float*)in, (float*)out);
    } else {
        const long n = (long)B * H * W * C;
        if (dtype == UIA_BF16) hipLaunchKernelGGL(upsample_ac_bwd_kernel<bf16_t>, dim3(blocks(n)), dim3(256), 0, stream, B, H, W, C, f, sy, sx, (const bf16_t*)in, (bf16_t*)out);
        else hipLaunchKernelGGL(upsample_ac_bwd_kernel<float>, dim3(blocks(n)), dim3(256), 0, stream, B, H, W, C, f, sy, sx, (const float*)in, (float*)out);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_resize_aa_launch(hipStream_t stream, int dtype, int backward, int B, int C, int Hi, int Wi, int Ho, int Wo, const void* x, float* tmp, float* out,
                         const float* dout, void* dx) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_resize_aa: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(B > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "uia_resize_aa: sizes must be positive");
    UIA_CHECK_ARG((long)B * C * Hi * Wi < (1l << 40) && (long)B * C * Ho * Wo < (1l << 40), "uia_resize_aa: shape too large");
    UIA_CHECK_ARG(Hi <= 3 * Ho && Wi <= 3 * Wo, "uia_resize_aa: downscale %dx%d -> %dx%d beyond 3x (window over %d taps)", Hi, Wi, Ho, Wo, AA_MAX_TAPS);
    UIA_CHECK_ARG(tmp, "uia_resize_aa: null scratch (B·C·Hi·Wo floats)");
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
    const long planes = (long)B * C;
    if (!backward) {
        UIA_CHECK_ARG(x && out, "uia_resize_aa: null tensor");
        if (dtype == UIA_BF16) hipLaunchKernelGGL(aa_h_fwd_kernel<bf16_t>, dim3(blocks(planes * Hi * Wo)), dim3(256), 0, stream, B, C, Hi, Wi, Wo, sw, (const bf16_t*)x, tmp);
        else hipLaunchKernelGGL(aa_h_fwd_kernel<float>, dim3(blocks(planes * Hi * Wo)), dim3(256), 0, stream, B, C, Hi, Wi, Wo, sw, (const float*)x, tmp);
        UIA_CHECK_LAUNCH();
        hipLaunchKernelGGL(aa_v_fwd_kernel, dim3(blocks(planes * Ho * Wo)), dim3(256), 0, stream, planes, Hi, Ho, Wo, sh, tmp, out);
    } else {
        UIA_CHECK_ARG(dout && dx, "uia_resize_aa: null tensor");
        hipLaunchKernelGGL(aa_v_bwd_kernel, dim3(blocks(planes * Hi * Wo)), dim3(256), 0, stream, planes, Hi, Ho, Wo, sh, dout, tmp);
        UIA_CHECK_LAUNCH();
        if (dtype == UIA_BF16) hipLaunchKernelGGL(aa_h_bwd_kernel<bf16_t>, dim3(blocks((long)B * Hi * Wi * C)), dim3(256), 0, stream, B, C, Hi, Wi, Wo, sw, tmp, (bf16_t*)dx);
        else hipLaunchKernelGGL(aa_h_bwd_kernel<float>, dim3(blocks((long)B * Hi * Wi * C)), dim3(256), 0, stream, B, C, Hi, Wi, Wo, sw, tmp, (float*)dx);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}
