// unet_pool.hip — nn.MaxPool2d(2) of the baseline UNet's DownBlock on NHWC activations (channels innermost).
//
// Replaces: nn.MaxPool2d(2) (the reference's src/third_party/unet.py:29), forward and backward.
//
// One thread per 2x2 window and channel group (V channels: 16 bytes when the channel count and the pointers allow, else one).  A trailing
// odd row / column belongs to no window: the forward ignores it, the backward writes zeros there, so the threads of the backward run over
// the ceil(H/2) x ceil(W/2) grid.  The backward recomputes the argmax from x (strict >, so ties stay with the first maximum in the order
// (0,0), (0,1), (1,0), (1,1), as PyTorch) and writes every element of dx: no atomics, no memset.  The running maximum starts from the
// window's first element.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

template <typename T, int V> struct Vec { T v[V]; } __attribute__((aligned(sizeof(T) * V)));

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(int B, int H, int W, int C, const T* __restrict__ x, T* __restrict__ y) {
    const int Ho = H / 2, Wo = W / 2, Cv = C / V;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Ho * Wo * Cv) return;
    const int cv = (int)(i % Cv);
    const long pix = i / Cv;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    const T* p = x + (((long)b * H + 2 * yo) * W + 2 * xo) * C + (long)cv * V;
    const Vec<T, V> a = *(const Vec<T, V>*)p, b1 = *(const Vec<T, V>*)(p + C), c = *(const Vec<T, V>*)(p + (long)W * C),
                    d = *(const Vec<T, V>*)(p + (long)W * C + C);
    Vec<T, V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        float m = to_f32(a.v[e]);
        T r = a.v[e];
        if (to_f32(b1.v[e]) > m) { m = to_f32(b1.v[e]); r = b1.v[e]; }
        if (to_f32(c.v[e]) > m) { m = to_f32(c.v[e]); r = c.v[e]; }
        if (to_f32(d.v[e]) > m) { m = to_f32(d.v[e]); r = d.v[e]; }
        o.v[e] = r;
    }
    *(Vec<T, V>*)(y + pix * C + (long)cv * V) = o;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(int B, int H, int W, int C, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx) {
    const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2, Cv = C / V;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Hc * Wc * Cv) return;
    const int cv = (int)(i % Cv);
    const long pix = i / Cv;
    const int xo = (int)(pix % Wc), yo = (int)((pix / Wc) % Hc), b = (int)(pix / ((long)Wc * Hc));
    const long base = (((long)b * H + 2 * yo) * W + 2 * xo) * C + (long)cv * V;
    Vec<T, V> o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) o[t].v[e] = (T)0.f;
    const bool whole = yo < Ho && xo < Wo;                // a complete window; otherwise only the trailing row / column's zeros
    if (whole) {
        const T* p = x + base;
        const Vec<T, V> w4[4] = {*(const Vec<T, V>*)p, *(const Vec<T, V>*)(p + C), *(const Vec<T, V>*)(p + (long)W * C), *(const Vec<T, V>*)(p + (long)W * C + C)};
        const Vec<T, V> g = *(const Vec<T, V>*)(dy + (((long)b * Ho + yo) * Wo + xo) * C + (long)cv * V);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float m = to_f32(w4[0].v[e]);
            int arg = 0;
#pragma unroll
            for (int t = 1; t < 4; ++t)
                if (to_f32(w4[t].v[e]) > m) { m = to_f32(w4[t].v[e]); arg = t; }
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (arg == t) o[t].v[e] = g.v[e];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int yy = 2 * yo + (t >> 1), xx = 2 * xo + (t & 1);
        if (yy < H && xx < W) *(Vec<T, V>*)(dx + base + ((long)(t >> 1) * W + (t & 1)) * C) = o[t];
    }
}

template <typename T, int V>
void launch(hipStream_t stream, int backward, int B, int H, int W, int C, const void* x, const void* dy, void* out) {
    if (backward) {
        const long n = (long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C / V);
        hipLaunchKernelGGL((maxpool2_bwd_kernel<T, V>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, H, W, C, (const T*)x, (const T*)dy, (T*)out);
    } else {
        const long n = (long)B * (H / 2) * (W / 2) * (C / V);
        hipLaunchKernelGGL((maxpool2_fwd_kernel<T, V>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, H, W, C, (const T*)x, (T*)out);
    }
}

}  // namespace

int uia_maxpool2_launch(hipStream_t stream, int dtype, int backward, int B, int H, int W, int C, const void* x, const void* dy, void* out) {
    const char* fn = backward ? "uia_maxpool2_bwd" : "uia_maxpool2_fwd";
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "%s: dtype must be UIA_F32 or UIA_BF16", fn);
    UIA_CHECK_ARG(B > 0 && C > 0 && H >= 2 && W >= 2, "%s: B=%d H=%d W=%d C=%d: positive sizes and a grid of at least 2x2 are required", fn, B, H, W, C);
    UIA_CHECK_ARG((long)B * H * W * C < (1l << 40), "%s: shape too large", fn);
    UIA_CHECK_ARG(x && out && (!backward || dy), "%s: null tensor", fn);
    const int V = dtype == UIA_BF16 ? 8 : 4;
    const bool vec = C % V == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)out) & 15) == 0;
    if (dtype == UIA_BF16) {
        if (vec) launch<bf16_t, 8>(stream, backward, B, H, W, C, x, dy, out);
        else launch<bf16_t, 1>(stream, backward, B, H, W, C, x, dy, out);
    } else {
        if (vec) launch<float, 4>(stream, backward, B, H, W, C, x, dy, out);
        else launch<float, 1>(stream, backward, B, H, W, C, x, dy, out);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}
