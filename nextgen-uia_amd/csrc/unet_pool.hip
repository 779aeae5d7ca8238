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

// ================================================================ the ResNet baseline's pools and layout helpers (src/third_party/resnet.py)
// nn.MaxPool2d(kernel 3, stride 2, padding 1) on NHWC x [B,H,W,C] -> y [B,Ho,Wo,C], Ho = (H − 1)/2 + 1.  The padding is −∞: a window takes the
// maximum of the elements that lie inside the grid, so an all-negative window returns its maximum (the running maximum starts from the
// window's first inside element; every window holds at least its centre).  Backward as a gather: one thread per input pixel and channel
// group looks at the at most four windows that cover it (two per axis for an odd coordinate, one for an even one), recomputes each
// window's argmax (strict >: ties stay with the first maximum in row-major window order, as PyTorch), adds dy of the windows it wins in
// window order in fp32 and writes every element of dx: no atomics, no memset.  Inputs are finite: NaN ordering is not part of the contract.
namespace {

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(int B, int H, int W, int C, const T* __restrict__ x, T* __restrict__ y) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Cv = C / V;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Ho * Wo * Cv) return;
    const int cv = (int)(i % Cv);
    const long pix = i / Cv;
    const int xo = (int)(pix % Wo), yo = (int)((pix / Wo) % Ho), b = (int)(pix / ((long)Wo * Ho));
    Vec<T, V> o;
    float m[V];
    bool first = true;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = 2 * yo + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = 2 * xo + dx;
            if (xx < 0 || xx >= W) continue;
            const Vec<T, V> a = *(const Vec<T, V>*)(x + (((long)b * H + yy) * W + xx) * C + (long)cv * V);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float f = to_f32(a.v[e]);
                if (first || f > m[e]) { m[e] = f; o.v[e] = a.v[e]; }
            }
            first = false;
        }
    }
    *(Vec<T, V>*)(y + pix * C + (long)cv * V) = o;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool3s2_bwd_kernel(int B, int H, int W, int C, const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Cv = C / V;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * H * W * Cv) return;
    const int cv = (int)(i % Cv);
    const long pix = i / Cv;
    const int xi = (int)(pix % W), yi = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    float g[V];
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    // windows yo with 2·yo − 1 <= yi <= 2·yo + 1
    const int yo0 = yi / 2, yo1 = (yi + 1) / 2, xo0 = xi / 2, xo1 = (xi + 1) / 2;
    for (int yo = yo0; yo <= yo1; ++yo) {
        if (yo >= Ho) continue;
        for (int xo = xo0; xo <= xo1; ++xo) {
            if (xo >= Wo) continue;
            float m[V];
            bool mine[V];
            bool first = true;
            for (int ddy = -1; ddy <= 1; ++ddy) {
                const int yy = 2 * yo + ddy;
                if (yy < 0 || yy >= H) continue;
                for (int ddx = -1; ddx <= 1; ++ddx) {
                    const int xx = 2 * xo + ddx;
                    if (xx < 0 || xx >= W) continue;
                    const Vec<T, V> a = *(const Vec<T, V>*)(x + (((long)b * H + yy) * W + xx) * C + (long)cv * V);
                    const bool me = yy == yi && xx == xi;
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float f = to_f32(a.v[e]);
                        if (first || f > m[e]) { m[e] = f; mine[e] = me; }
                    }
                    first = false;
                }
            }
            const Vec<T, V> d = *(const Vec<T, V>*)(dy + (((long)b * Ho + yo) * Wo + xo) * C + (long)cv * V);
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (mine[e]) g[e] += to_f32(d.v[e]);
        }
    }
    Vec<T, V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) o.v[e] = from_f32<T>(g[e]);
    *(Vec<T, V>*)(dx + pix * C + (long)cv * V) = o;
}

template <typename T, int V>
void launch3(hipStream_t stream, int backward, int B, int H, int W, int C, const void* x, const void* dy, void* out) {
    if (backward) {
        const long n = (long)B * H * W * (C / V);
        hipLaunchKernelGGL((maxpool3s2_bwd_kernel<T, V>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, H, W, C, (const T*)x, (const T*)dy, (T*)out);
    } else {
        const long n = (long)B * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (C / V);
        hipLaunchKernelGGL((maxpool3s2_fwd_kernel<T, V>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, H, W, C, (const T*)x, (T*)out);
    }
}

// global average pool: one thread per (image, channel) adds the H·W pixels in pixel order in fp32 (neighbouring threads read neighbouring
// channels), then divides once
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(int B, int HW, int C, const T* __restrict__ x, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int c = (int)(i % C);
    const long b = i / C;
    const T* p = x + b * HW * C + c;
    float s = 0.f;
    for (int k = 0; k < HW; ++k) s += to_f32(p[(long)k * C]);
    out[i] = s / (float)HW;
}
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(long n, int HW, int C, const float* __restrict__ dout, T* __restrict__ dx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const long b = i / ((long)HW * C);
    dx[i] = from_f32<T>(dout[b * C + c] / (float)HW);
}

// fp32 NCHW [B,Cin,H,W] -> NHWC [B,H,W,Cout] of T: channel c < Cin copies channel c (Cin == 1: channel 0, for every c < rep), the rest is zero
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(long n, int Cin, int HW, int Cout, int rep, const float* __restrict__ x, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Cout);
    const long pix = i / Cout;
    const long b = pix / HW, p = pix - b * HW;
    float v = 0.f;
    if (c < rep) v = x[(b * Cin + (Cin == 1 ? 0 : c)) * HW + p];
    out[i] = from_f32<T>(v);
}

template <typename T>
__global__ __launch_bounds__(256) void add2_kernel(long n, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = from_f32<T>(to_f32(a[i]) + to_f32(b[i]));
}
template <typename T>
__global__ __launch_bounds__(256) void add2x8_kernel(long n8, const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float u[8], v[8];
    load8(a + 8 * i, u);
    load8(b + 8 * i, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] += v[e];
    store8(out + 8 * i, u);
}

}  // namespace

int uia_maxpool3s2_launch(hipStream_t stream, int dtype, int backward, int B, int H, int W, int C, const void* x, const void* dy, void* out) {
    const char* fn = backward ? "uia_maxpool3s2_bwd" : "uia_maxpool3s2_fwd";
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "%s: dtype must be UIA_F32 or UIA_BF16", fn);
    UIA_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "%s: B=%d H=%d W=%d C=%d must be positive", fn, B, H, W, C);
    UIA_CHECK_ARG((long)B * H * W * C < (1l << 40), "%s: shape too large", fn);
    UIA_CHECK_ARG(x && out && (!backward || dy), "%s: null tensor", fn);
    const int V = dtype == UIA_BF16 ? 8 : 4;
    const bool vec = C % V == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)out) & 15) == 0;
    if (dtype == UIA_BF16) {
        if (vec) launch3<bf16_t, 8>(stream, backward, B, H, W, C, x, dy, out);
        else launch3<bf16_t, 1>(stream, backward, B, H, W, C, x, dy, out);
    } else {
        if (vec) launch3<float, 4>(stream, backward, B, H, W, C, x, dy, out);
        else launch3<float, 1>(stream, backward, B, H, W, C, x, dy, out);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_avgpool_launch(hipStream_t stream, int dtype, int backward, int B, int H, int W, int C, const void* x, float* pooled, void* dx) {
    const char* fn = backward ? "uia_avgpool_bwd" : "uia_avgpool_fwd";
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "%s: dtype must be UIA_F32 or UIA_BF16", fn);
    UIA_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && (long)H * W < (1l << 30), "%s: B=%d H=%d W=%d C=%d must be positive", fn, B, H, W, C);
    UIA_CHECK_ARG((long)B * H * W * C < (1l << 40), "%s: shape too large", fn);
    UIA_CHECK_ARG(pooled && (backward ? dx != nullptr : x != nullptr), "%s: null tensor", fn);
    const int HW = H * W;
    if (backward) {
        const long n = (long)B * HW * C;
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(avgpool_bwd_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, HW, C, pooled, (bf16_t*)dx);
        else
            hipLaunchKernelGGL(avgpool_bwd_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, HW, C, pooled, (float*)dx);
    } else {
        const long n = (long)B * C;
        if (dtype == UIA_BF16)
            hipLaunchKernelGGL(avgpool_fwd_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, HW, C, (const bf16_t*)x, pooled);
        else
            hipLaunchKernelGGL(avgpool_fwd_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, HW, C, (const float*)x, pooled);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_nchw_to_nhwc_launch(hipStream_t stream, int dtype, int B, int Cin, int H, int W, int Cout, int rep, const float* x, void* out) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_nchw_to_nhwc: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, "uia_nchw_to_nhwc: B=%d Cin=%d H=%d W=%d Cout=%d must be positive", B, Cin, H, W, Cout);
    UIA_CHECK_ARG(rep >= 0 && rep <= Cout && (rep <= Cin || Cin == 1), "uia_nchw_to_nhwc: %d filled channels from %d sources into %d", rep, Cin, Cout);
    UIA_CHECK_ARG((long)B * H * W * (Cout > Cin ? Cout : Cin) < (1l << 40) && (long)H * W < (1l << 31), "uia_nchw_to_nhwc: shape too large");
    UIA_CHECK_ARG(x && out, "uia_nchw_to_nhwc: null tensor");
    const long n = (long)B * H * W * Cout;
    if (dtype == UIA_BF16)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, Cin, H * W, Cout, rep, x, (bf16_t*)out);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, Cin, H * W, Cout, rep, x, (float*)out);
    UIA_CHECK_LAUNCH();
    return 0;
}

int uia_add2_launch(hipStream_t stream, int dtype, long n, const void* a, const void* b, void* out) {
    UIA_CHECK_ARG(dtype == UIA_F32 || dtype == UIA_BF16, "uia_add2: dtype must be UIA_F32 or UIA_BF16");
    UIA_CHECK_ARG(n > 0 && n < (1l << 40), "uia_add2: n=%ld out of range", n);
    UIA_CHECK_ARG(a && b && out, "uia_add2: null tensor");
    const bool vec = n % 8 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0;
    const long t = vec ? n / 8 : n;
    const dim3 grid((unsigned)((t + 255) / 256));
    if (dtype == UIA_BF16) {
        if (vec) hipLaunchKernelGGL(add2x8_kernel<bf16_t>, grid, dim3(256), 0, stream, t, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out);
        else hipLaunchKernelGGL(add2_kernel<bf16_t>, grid, dim3(256), 0, stream, t, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out);
    } else {
        if (vec) hipLaunchKernelGGL(add2x8_kernel<float>, grid, dim3(256), 0, stream, t, (const float*)a, (const float*)b, (float*)out);
        else hipLaunchKernelGGL(add2_kernel<float>, grid, dim3(256), 0, stream, t, (const float*)a, (const float*)b, (float*)out);
    }
    UIA_CHECK_LAUNCH();
    return 0;
}
