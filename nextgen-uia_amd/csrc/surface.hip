// surface.hip — the two surface-distance metrics of the segmentation entry points' MetricAccumulator (reference src/utils/tools.py:185-206:
// MONAI compute_hausdorff_distance(percentile=95) and compute_average_surface_distance, include_background=False, spacing=None), for the binary case.
// Per image b, with P = argmax(logits[b]) == 1 (torch's rules: a tie goes to class 0, NaN is the maximum) and G = label[b, 0] > 0:
//   E(M) = M & ~erode(M), the 4-neighbour erosion with out-of-image pixels as background (scipy binary_erosion after MONAI's margin-1 crop);
//   d(A→B) = the exact Euclidean distance from every pixel of E(A) to the nearest pixel of E(B), as float32(sqrt(double(integer squared distance)));
//   hd = max(q(d(P→G)), q(d(G→P))) with q = torch.quantile at percentile / 100 (float32 rank, lerp of two exact order statistics; percentile 0 is the
//   maximum, as in MONAI); asd = mean of d(P→G).
// An empty P or G gives NaN for both.  Five launches over a caller-owned workspace:
//   edge_kernel     one thread per pixel: E(P), E(G) as bytes;
//   column_kernel   one thread per (image, map, column): the vertical distance to the map's nearest edge pixel in that column (uint16, NO_EDGE if none);
//   row_kernel      one wave per (image, direction, row): the row of column distances of the target map in LDS; each query edge pixel scans outward from its
//                   column and stops once dx² alone reaches its best g² + dx² (exact; at most W steps);
//   select_kernel   one workgroup per (image, direction): count, fp64 sum in a fixed order, and the two order statistics of the percentile by a two-level
//                   radix select on the integer squared distances in LDS (integer LDS atomics only);
//   final_kernel    one thread per image: hd and asd from the two directions' records, ordinary stores.
// No float atomics, fixed summation order: two calls on one input agree bit for bit.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int SURF_MAXHW = 1024;
constexpr int SURF_MAXB = 1 << 20;
constexpr unsigned short NO_EDGE = 0xFFFF;         // column distance: no edge pixel of the target in this column
constexpr unsigned NOT_QUERY = 0xFFFFFFFFu;        // squared-distance map: not an edge pixel of the query map
constexpr unsigned FAR = (1u << 21) - 1;           // no edge pixel of the target at all; every real value is <= 2·1023² = 2 093 058 < FAR
constexpr int ROW_WAVES = 4;
constexpr int SEL_THREADS = 1024;
constexpr int HI_BINS = 2048;                      // value >> 10 (21-bit values)
constexpr int LO_BINS = 1024;                      // value & 1023

struct DirRecord {                                 // one per (image, direction) in the workspace
    double sum;                                    // Σ float32 distances, fp64, fixed order
    double q;                                      // the percentile of the float32 distances
    long long n;                                   // edge pixels of the query map
};

struct SurfLayout {
    size_t edges, cold, dist, rec, total;
};

SurfLayout surf_layout(int B, int H, int W) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t px = (size_t)B * 2 * H * W;
    SurfLayout l;
    l.edges = 0;
    l.cold = up(px);                               // uint8 [B][2][H][W]: E(P), E(G)
    l.dist = l.cold + up(px * sizeof(unsigned short));     // uint16 [B][2][H][W]: column distances of the target of direction 0 (E(G)) and 1 (E(P))
    l.rec = l.dist + up(px * sizeof(unsigned));    // uint32 [B][2][H][W]: squared distances at the query's edge pixels
    l.total = l.rec + up((size_t)B * 2 * sizeof(DirRecord));
    return l;
}

// class 1 wins torch.argmax over (l0, l1): l0 is not NaN and (l1 is NaN or l1 > l0)
__device__ __forceinline__ bool pred_at(const float* __restrict__ lg, size_t plane, size_t i) {
    const float l0 = lg[i], l1 = lg[plane + i];
    return !(l0 != l0) && ((l1 != l1) || l1 > l0);
}

__global__ __launch_bounds__(256) void edge_kernel(int B, int H, int W, const float* __restrict__ logits, const float* __restrict__ label,
                                                   unsigned char* __restrict__ edges) {
    const size_t HW = (size_t)H * W;
    const size_t total = (size_t)B * HW;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t b = e / HW, p = e % HW;
        const int y = (int)(p / W), x = (int)(p % W);
        const float* lg = logits + b * 2 * HW;
        const float* lb = label + b * HW;
        const bool up = y > 0, dn = y + 1 < H, lf = x > 0, rt = x + 1 < W;
        // an edge pixel: in the mask with a 4-neighbour outside it (out of the image counts as outside)
        const bool mp = pred_at(lg, HW, p);
        const bool ip = up && dn && lf && rt && pred_at(lg, HW, p - W) && pred_at(lg, HW, p + W) && pred_at(lg, HW, p - 1) && pred_at(lg, HW, p + 1);
        const bool mg = lb[p] > 0.f;
        const bool ig = up && dn && lf && rt && lb[p - W] > 0.f && lb[p + W] > 0.f && lb[p - 1] > 0.f && lb[p + 1] > 0.f;
        edges[(b * 2 + 0) * HW + p] = mp && !ip;
        edges[(b * 2 + 1) * HW + p] = mg && !ig;
    }
}

// thread (b, dir, x): cold[b][dir][.][x] = |y - y'| to the nearest edge pixel y' of column x of the target map of direction dir (dir 0: E(G), dir 1: E(P))
__global__ __launch_bounds__(256) void column_kernel(int B, int H, int W, const unsigned char* __restrict__ edges, unsigned short* __restrict__ cold) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)B * 2 * W) return;
    const int x = (int)(t % W);
    const size_t bd = t / W, b = bd / 2, dir = bd % 2;
    const size_t HW = (size_t)H * W;
    const unsigned char* src = edges + (b * 2 + (1 - dir)) * HW + x;
    unsigned short* dst = cold + bd * HW + x;
    int last = -1;
    for (int y = 0; y < H; ++y) {
        if (src[(size_t)y * W]) last = y;
        dst[(size_t)y * W] = last < 0 ? NO_EDGE : (unsigned short)(y - last);
    }
    int next = -1;
    for (int y = H - 1; y >= 0; --y) {
        if (src[(size_t)y * W]) next = y;
        if (next >= 0) {
            const unsigned short d = (unsigned short)(next - y);
            const unsigned short cur = dst[(size_t)y * W];
            if (d < cur) dst[(size_t)y * W] = d;
        }
    }
}

// wave w of the workgroup: row r = (b·2 + dir)·H + y.  dist[r][x] = min over x' of cold[r][x']² + (x - x')² for every edge pixel x of the query map, else NOT_QUERY.
__global__ __launch_bounds__(64 * ROW_WAVES) void row_kernel(int B, int H, int W, const unsigned char* __restrict__ edges,
                                                             const unsigned short* __restrict__ cold, unsigned* __restrict__ dist) {
    __shared__ unsigned short g[ROW_WAVES][SURF_MAXHW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t r = (size_t)blockIdx.x * ROW_WAVES + wave;
    const bool valid = r < (size_t)B * 2 * H;
    const size_t bd = r / H, y = r % H;
    const size_t HW = (size_t)H * W;
    unsigned short* gr = g[wave];
    if (valid) {
        const unsigned short* src = cold + bd * HW + y * W;
        for (int x = lane; x < W; x += 64) gr[x] = src[x];
    }
    __syncthreads();
    if (!valid) return;
    const unsigned char* q = edges + bd * HW + y * W;        // query map of direction dir = bd % 2: E(P) for 0, E(G) for 1 (layout [b][map], map = dir)
    unsigned* out = dist + bd * HW + y * W;
    for (int x = lane; x < W; x += 64) {
        unsigned best = NOT_QUERY;
        if (q[x]) {
            best = FAR;
            const unsigned g0 = gr[x];
            if (g0 != NO_EDGE) best = g0 * g0;
            for (int d = 1; (unsigned)(d * d) < best && (x - d >= 0 || x + d < W); ++d) {
                const unsigned dd = (unsigned)(d * d);
                if (x - d >= 0) {
                    const unsigned gl = gr[x - d];
                    if (gl != NO_EDGE && gl * gl + dd < best) best = gl * gl + dd;
                }
                if (x + d < W) {
                    const unsigned gh = gr[x + d];
                    if (gh != NO_EDGE && gh * gh + dd < best) best = gh * gh + dd;
                }
            }
        }
        out[x] = best;
    }
}

__device__ __forceinline__ float dist_of(unsigned v) { return (float)sqrt((double)v); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Exclusive prefix of `bins` counters (bins = k·SEL_THREADS) held in LDS; returns, through *bin / *before, the bin that holds rank k (0-based) and the number
// of values in the bins below it.  Thread t owns bins [t·per, (t+1)·per).
__device__ void find_rank(const unsigned* hist, int bins, long long k, long long* scan, int* bin, long long* before) {
    const int tid = threadIdx.x, per = bins / SEL_THREADS;
    if (tid == 0) {                                         // defined even if no thread finds k (k < the total is the caller's contract)
        *bin = 0;
        *before = 0;
    }
    long long own = 0;
    for (int i = 0; i < per; ++i) own += hist[tid * per + i];
    scan[tid] = own;
    __syncthreads();
    for (int d = 1; d < SEL_THREADS; d <<= 1) {             // Hillis–Steele inclusive scan
        const long long o = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += o;
        __syncthreads();
    }
    long long acc = scan[tid] - own;                        // values in the bins below this thread's
    if (acc <= k && k < scan[tid]) {
        for (int i = 0; i < per; ++i) {
            const unsigned c = hist[tid * per + i];
            if (k < acc + c) {
                *bin = tid * per + i;
                *before = acc;
                break;
            }
            acc += c;
        }
    }
    __syncthreads();
}

// workgroup (b, dir) over dist[b][dir]: n, Σ d (fp64), and q = lerp(s[lo], s[hi], w) at rank r = q·(n - 1) in float32 (torch.quantile, linear).
__global__ __launch_bounds__(SEL_THREADS) void select_kernel(int H, int W, float quant, const unsigned* __restrict__ dist, DirRecord* __restrict__ rec) {
    __shared__ unsigned hist_hi[HI_BINS];
    __shared__ unsigned hist_lo[LO_BINS];
    __shared__ long long scan[SEL_THREADS];
    __shared__ double wsum[SEL_THREADS / 64];
    __shared__ long long wcnt[SEL_THREADS / 64];
    __shared__ int sel_bin;
    __shared__ long long sel_before;
    __shared__ unsigned next_min;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t HW = (size_t)H * W;
    const unsigned* v = dist + (size_t)blockIdx.x * HW;
    for (int i = tid; i < HI_BINS; i += SEL_THREADS) hist_hi[i] = 0;
    for (int i = tid; i < LO_BINS; i += SEL_THREADS) hist_lo[i] = 0;
    if (tid == 0) next_min = 0xFFFFFFFFu;
    __syncthreads();
    // pass 1: count, fp64 sum (per thread in index order, then waves in order), histogram of the high bits
    double s = 0.0;
    long long n = 0;
    for (size_t i = tid; i < HW; i += SEL_THREADS) {
        const unsigned a = v[i];
        if (a != NOT_QUERY) {
            ++n;
            s += (double)dist_of(a);
            atomicAdd(&hist_hi[a >> 10], 1u);
        }
    }
    s = wave_sum_f64(s);
    n = wave_sum_i64(n);
    if (lane == 0) {
        wsum[wave] = s;
        wcnt[wave] = n;
    }
    __syncthreads();
    double tot = 0.0;
    long long cnt = 0;
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
        tot += wsum[w];
        cnt += wcnt[w];
    }
    DirRecord* out = rec + blockIdx.x;
    if (cnt == 0) {                                         // block-uniform
        if (tid == 0) {
            out->sum = 0.0;
            out->q = __builtin_nan("");
            out->n = 0;
        }
        return;
    }
    const float rank = __fmul_rn(quant, (float)(cnt - 1));
    const float rf = floorf(rank);
    const long long klo = (long long)rf, khi = (long long)ceilf(rank);
    const float wgt = __fsub_rn(rank, rf);
    // pass 2: the high bin of rank klo, then the histogram of the low bits inside it
    find_rank(hist_hi, HI_BINS, klo, scan, &sel_bin, &sel_before);
    const unsigned hb = (unsigned)sel_bin;
    const long long below_hi = sel_before;
    for (size_t i = tid; i < HW; i += SEL_THREADS) {
        const unsigned a = v[i];
        if (a != NOT_QUERY && (a >> 10) == hb) atomicAdd(&hist_lo[a & 1023], 1u);
    }
    __syncthreads();
    find_rank(hist_lo, LO_BINS, klo - below_hi, scan, &sel_bin, &sel_before);
    const unsigned vlo = hb << 10 | (unsigned)sel_bin;
    const long long le = below_hi + sel_before + hist_lo[sel_bin];     // values <= vlo
    unsigned vhi = vlo;
    if (khi > klo && le <= khi) {                           // rank khi holds the smallest value above vlo: pass 3
        unsigned m = 0xFFFFFFFFu;
        for (size_t i = tid; i < HW; i += SEL_THREADS) {
            const unsigned a = v[i];
            if (a != NOT_QUERY && a > vlo && a < m) m = a;
        }
        atomicMin(&next_min, m);
        __syncthreads();
        vhi = next_min;
    }
    if (tid == 0) {
        // torch.lerp(a, b, w): w < 0.5 ? a + w·(b - a) : b - (b - a)·(1 - w), each step rounded to float32
        const float a = dist_of(vlo), bb = dist_of(vhi);
        const float diff = __fsub_rn(bb, a);
        const float qv = fabsf(wgt) < 0.5f ? __fadd_rn(a, __fmul_rn(wgt, diff)) : __fsub_rn(bb, __fmul_rn(diff, __fsub_rn(1.f, wgt)));
        out->sum = tot;
        out->q = (double)qv;
        out->n = cnt;
    }
}

__global__ __launch_bounds__(256) void final_kernel(int B, const DirRecord* __restrict__ rec, double* __restrict__ hd, double* __restrict__ asd) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const DirRecord pg = rec[2 * b], gp = rec[2 * b + 1];
    const double nan = __builtin_nan("");
    const bool ok = pg.n > 0 && gp.n > 0;
    hd[b] = ok ? (pg.q > gp.q ? pg.q : gp.q) : nan;
    asd[b] = ok ? pg.sum / (double)pg.n : nan;
}

}  // namespace

size_t uia_surface_ws_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return surf_layout(B, H, W).total;
}

int uia_surface_launch(hipStream_t stream, int B, int H, int W, const float* logits, const float* label, float percentile, void* ws, size_t ws_bytes,
                       double* hd, double* asd) {
    UIA_CHECK_ARG(B >= 1 && B <= SURF_MAXB && H >= 1 && H <= SURF_MAXHW && W >= 1 && W <= SURF_MAXHW,
                  "uia_surface_distances: bad shape B=%d H=%d W=%d (1 <= B <= %d, 1 <= H, W <= %d)", B, H, W, SURF_MAXB, SURF_MAXHW);
    UIA_CHECK_ARG(logits && label && ws && hd && asd, "uia_surface_distances: null tensor");
    UIA_CHECK_ARG(percentile >= 0.f && percentile <= 100.f, "uia_surface_distances: percentile %g outside [0, 100]", (double)percentile);
    const SurfLayout l = surf_layout(B, H, W);
    UIA_CHECK_ARG(ws_bytes >= l.total, "uia_surface_distances: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    char* base = (char*)ws;
    unsigned char* edges = (unsigned char*)(base + l.edges);
    unsigned short* cold = (unsigned short*)(base + l.cold);
    unsigned* dist = (unsigned*)(base + l.dist);
    DirRecord* rec = (DirRecord*)(base + l.rec);
    const size_t px = (size_t)B * H * W;
    const size_t eg = (px + 255) / 256;
    hipLaunchKernelGGL(edge_kernel, dim3((unsigned)(eg < 4096 ? eg : 4096)), dim3(256), 0, stream, B, H, W, logits, label, edges);
    hipLaunchKernelGGL(column_kernel, dim3((unsigned)(((size_t)B * 2 * W + 255) / 256)), dim3(256), 0, stream, B, H, W, edges, cold);
    hipLaunchKernelGGL(row_kernel, dim3((unsigned)(((size_t)B * 2 * H + ROW_WAVES - 1) / ROW_WAVES)), dim3(64 * ROW_WAVES), 0, stream, B, H, W, edges, cold, dist);
    // MONAI's _compute_percentile_hausdorff_distance: `if not percentile: return max` — percentile 0 is the plain (directed) Hausdorff distance, i.e. the
    // quantile at 1; otherwise torch.quantile(d, percentile / 100)
    const float quant = percentile == 0.f ? 1.f : (float)((double)percentile / 100.0);
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)(2 * B)), dim3(SEL_THREADS), 0, stream, H, W, quant, dist, rec);
    hipLaunchKernelGGL(final_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, B, rec, hd, asd);
    UIA_CHECK_LAUNCH();
    return 0;
}
