// retrieval.hip — image-text retrieval evaluation (the fifth step of the reference's BiomedCLIP pipeline, src/models/biomedclip/retrieval.py:329; its
// metric module src/utils/retrieval_metrics.py was never shipped, so the definitions below are this build's).
//
//   * uia_retrieval_ranks: for N paired feature rows img_i, txt_i (fp32 [N, E]) the scores s_ij = <a_i, b_j> (a, b the rows, L2-normalised with
//     F.normalize's eps 1e-12 when asked) are formed tile by tile on the exact fp32 MFMA and reduced in the tile's epilogue to rank counts against the
//     diagonal d_i = s_ii, in both directions at once:
//         gt_i2t[i] = #{ j != i : s_ij > d_i }     eq_i2t[i] = #{ j != i : s_ij == d_i }      (image i queries the texts: row i of the scores)
//         gt_t2i[j] = #{ i != j : s_ij > d_j }     eq_t2i[j] = #{ i != j : s_ij == d_j }      (text j queries the images: column j)
//     The N x N matrix is never written.  Ranks are OPTIMISTIC: rank = 1 + gt, the usual (sim > diag).sum() form; eq tells how many others tie with the
//     query's own pair.  IEEE comparisons: a NaN score is neither greater nor equal; a query whose own d is not finite gets gt = N - 1, eq = 0.
//   * uia_retrieval_stats: R@K (100 · #{rank <= K} / N), the median rank (numpy.median: the two middle values averaged for even N) and the mean rank of
//     one direction's gt, as an fp64 record on the device.  rsum, the sum of every R@K of both directions, is formed by the caller from two records.
//   * uia_retrieval_topk: each query's K <= 32 best gallery rows (queries [Q, E] against gallery [N, E], rectangular), from the same score tiles with a
//     selection epilogue instead of the counts; one total order (score descending, equal scores by index ascending, NaN last).  See "top-K listing" below.
//
// Position independence (the contract of the rank counts): the bits of s_ij depend only on the values of row i of img and row j of txt.
//   - v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain from C = 0 (one rounding per product, no wider accumulator), and every element of every
//     tile runs that same chain over k = 0 .. E-1 in order, whatever lane, wave, tile or grid position holds it.  k past E is loaded as 0 for BOTH operands
//     (by index), and fma(0, 0, acc) leaves acc's value as it is.
//   - the normalised row is computed once per row by one wave in a fixed order (lane-strided fmaf, then the fixed butterfly of wave_sum) and stored; tiles
//     read the stored row.
//   - d_i is taken from the tile path itself: a first pass runs the same main loop over the diagonal tiles and stores s_ii.  Duplicate captions therefore
//     give exact ties.
// Padding never counts: rows and columns past N are masked by INDEX in the epilogue (a zero-padded column scores 0, which beats a negative diagonal).
//
// Block: 128 x 128 scores, K step 32, four waves of 2 x 2 32x32x2 tiles (64 accumulator registers).  Operands go global -> registers -> LDS ([row][k], row
// stride 33 floats: the one-float-per-lane A/B fragment reads A[i = lane & 31][k = lane >> 5] are then conflict-free); the next K step's global loads are
// in flight during the MFMAs.  Epilogue: C/D map col = lane & 31, row = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5).  A row's count is the popcount of one
// half of a wave ballot; a column's is a per-lane sum plus its partner lane.  Both go to LDS counters with integer atomics, then one integer atomicAdd per
// row and per column of the tile to global memory (skipped when the count is 0).  Integer atomics commute: the result is deterministic.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int RT_MAXN = 1 << 24;
constexpr int RT_MAXE = 4096;
constexpr int RT_TILE = 128;                       // scores per block edge
constexpr int RT_BK = 32;
constexpr int RT_LD = RT_BK + 1;                   // LDS row stride in floats
constexpr int RT_THREADS = 256;
constexpr int RT_GRID_Y = 32768;                  // row tiles per grid z-slice

struct RankLayout {
    size_t diag, an, bn, total;
};

RankLayout rank_layout(int N, int E) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    RankLayout l;
    l.diag = 0;                                    // float [N]: d_i = s_ii
    l.an = up((size_t)N * sizeof(float));          // float [N][E]: normalised img rows (normalize != 0 only)
    l.bn = l.an + up((size_t)N * E * sizeof(float));
    l.total = l.bn + up((size_t)N * E * sizeof(float));
    return l;
}

// One wave per row: dst = src / max(||src||, 1e-12) (F.normalize; the eps of infonce.hip).  Rows 0 .. NA-1 are a's, NA .. NA+NB-1 b's.
__global__ __launch_bounds__(256) void rt_normalize_kernel(int NA, int NB, int E, const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ an, float* __restrict__ bn) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)NA + (size_t)NB) return;
    const float* src = row < (size_t)NA ? a + row * E : b + (row - NA) * E;
    float* dst = row < (size_t)NA ? an + row * E : bn + (row - NA) * E;
    float s = 0.f;
    for (int e = lane; e < E; e += 64) s = fmaf(src[e], src[e], s);
    const float nrm = fmaxf(sqrtf(wave_sum(s)), 1e-12f);
    for (int e = lane; e < E; e += 64) dst[e] = src[e] / nrm;
}

// 4 float4 per thread and operand: rows idx >> 3, k quad idx & 7 of the 128 x 32 slab, idx = tid + 256·q.  Rows past N and k past E load as zero.
__device__ __forceinline__ void rt_fetch(const float* __restrict__ src, int N, int E, size_t row0, int k0, int tid, f32x4 (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = tid + RT_THREADS * q;
        const size_t r = row0 + (size_t)(idx >> 3);
        const int k = k0 + (idx & 7) * 4;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        v[q] = (r < (size_t)N && k < E) ? *(const f32x4*)(src + r * E + k) : z;       // E % 4 == 0: a quad is wholly inside or outside
    }
}

__device__ __forceinline__ void rt_stage(float* __restrict__ lds, int tid, const f32x4 (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = tid + RT_THREADS * q;
        float* p = lds + (idx >> 3) * RT_LD + (idx & 7) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = v[q][e];
    }
}

// acc[m][n] = the wave's 32 x 32 score sub-tiles of the block (m0, n0): rows m0 + wm·64 + m·32 + .., columns n0 + wn·64 + n·32 + ..
// Each element is fma(a_{E-1}, b_{E-1}, ... fma(a_0, b_0, 0)) in k order.  A has NA rows, B has NB.  Ends with the block past its last LDS read.
__device__ __forceinline__ void rt_tile_scores(const float* __restrict__ A, const float* __restrict__ B, int NA, int NB, int E, size_t m0, size_t n0,
                                               float* As, float* Bs, f32x16 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
    const float* ap = As + (wm * 64 + (lane & 31)) * RT_LD + (lane >> 5);
    const float* bp = Bs + (wn * 64 + (lane & 31)) * RT_LD + (lane >> 5);
    f32x4 va[4], vb[4];
    rt_fetch(A, NA, E, m0, 0, tid, va);
    rt_fetch(B, NB, E, n0, 0, tid, vb);
    for (int k0 = 0; k0 < E; k0 += RT_BK) {
        __syncthreads();                                           // the previous step's fragment reads are done
        rt_stage(As, tid, va);
        rt_stage(Bs, tid, vb);
        __syncthreads();
        if (k0 + RT_BK < E) {
            rt_fetch(A, NA, E, m0, k0 + RT_BK, tid, va);
            rt_fetch(B, NB, E, n0, k0 + RT_BK, tid, vb);
        }
#pragma unroll
        for (int kk = 0; kk < RT_BK / 2; ++kk) {
            const float a0 = ap[2 * kk], a1 = ap[32 * RT_LD + 2 * kk];
            const float b0 = bp[2 * kk], b1 = bp[32 * RT_LD + 2 * kk];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool rt_not_finite(float x) { return !(fabsf(x) < __builtin_inff()); }

// First pass: block t computes the diagonal tile (t, t) and stores d_i = s_ii.
__global__ __launch_bounds__(RT_THREADS) void rt_diag_kernel(int N, int E, const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ diag) {
    __shared__ float As[RT_TILE * RT_LD];
    __shared__ float Bs[RT_TILE * RT_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const size_t t0 = (size_t)blockIdx.x * RT_TILE;
    f32x16 acc[2][2];
    rt_tile_scores(A, B, N, N, E, t0, t0, As, Bs, acc);
    if (wm != wn) return;                                          // the diagonal of the block lies in the waves (0, 0) and (1, 1), sub-tiles m == n
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int c = lane & 31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const size_t g = t0 + (size_t)(wm * 64 + m * 32 + row);
            if (row == c && g < (size_t)N) diag[g] = acc[m][m][r];
        }
    }
}

// Second pass: block (x, y, z) owns the tile (tm = z·gridDim.y + y, tn = x); z exists only because a grid's y is limited to 65535.
__global__ __launch_bounds__(RT_THREADS, 2) void rt_rank_kernel(int N, int E, const float* __restrict__ A, const float* __restrict__ B,
                                                             const float* __restrict__ diag, int* __restrict__ gt_r, int* __restrict__ eq_r,
                                                             int* __restrict__ gt_c, int* __restrict__ eq_c) {
    __shared__ float As[RT_TILE * RT_LD];
    __shared__ float Bs[RT_TILE * RT_LD];
    __shared__ float drow[RT_TILE], dcol[RT_TILE];
    __shared__ int cnt[4][RT_TILE];                                // row gt, row eq, column gt, column eq
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, c = lane & 31;
    const int tiles = (N + RT_TILE - 1) / RT_TILE;
    const int tm = blockIdx.z * gridDim.y + blockIdx.y;
    if (tm >= tiles) return;
    const size_t m0 = (size_t)tm * RT_TILE, n0 = (size_t)blockIdx.x * RT_TILE;
    if (tid < RT_TILE) {
        drow[tid] = m0 + tid < (size_t)N ? diag[m0 + tid] : 0.f;
        cnt[0][tid] = 0;
        cnt[1][tid] = 0;
    } else {
        const int u = tid - RT_TILE;
        dcol[u] = n0 + u < (size_t)N ? diag[n0 + u] : 0.f;
        cnt[2][u] = 0;
        cnt[3][u] = 0;
    }
    f32x16 acc[2][2];
    rt_tile_scores(A, B, N, N, E, m0, n0, As, Bs, acc);         // its barriers order the writes above before the reads below
    int cg[2] = {0, 0}, ce[2] = {0, 0};
    float dj[2];
    bool okj[2], badj[2];
    size_t gj[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int lc = wn * 64 + n * 32 + c;
        gj[n] = n0 + lc;
        dj[n] = dcol[lc];
        okj[n] = gj[n] < (size_t)N;
        badj[n] = rt_not_finite(dj[n]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const size_t gi = m0 + lr;
            const float di = drow[lr];
            const bool badi = rt_not_finite(di);
            int rg = 0, re = 0;                                // this lane's half-wave holds row lr: its count over the wave's 64 columns
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const float s = acc[m][n][r];
                const bool ok = okj[n] && gi < (size_t)N && gi != gj[n];          // by index: padding and the pair itself never count
                const bool pg = ok && (badi || s > di), pe = ok && !badi && s == di;
                const bool qg = ok && (badj[n] || s > dj[n]), qe = ok && !badj[n] && s == dj[n];
                cg[n] += qg;
                ce[n] += qe;
                const unsigned long long bg = __ballot(pg), be = __ballot(pe);
                rg += __popc(half ? (unsigned)(bg >> 32) : (unsigned)bg);
                if (be) re += __popc(half ? (unsigned)(be >> 32) : (unsigned)be);
            }
            if (c == 0) {
                if (rg) atomicAdd(&cnt[0][lr], rg);
                if (re) atomicAdd(&cnt[1][lr], re);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        cg[n] += __shfl_xor(cg[n], 32, 64);
        ce[n] += __shfl_xor(ce[n], 32, 64);
        if (half == 0) {
            const int lc = wn * 64 + n * 32 + c;
            if (cg[n]) atomicAdd(&cnt[2][lc], cg[n]);
            if (ce[n]) atomicAdd(&cnt[3][lc], ce[n]);
        }
    }
    __syncthreads();
    if (tid < RT_TILE) {
        const size_t g = m0 + tid;
        if (g < (size_t)N) {
            if (cnt[0][tid]) atomicAdd(&gt_r[g], cnt[0][tid]);
            if (cnt[1][tid]) atomicAdd(&eq_r[g], cnt[1][tid]);
        }
    } else {
        const int u = tid - RT_TILE;
        const size_t g = n0 + u;
        if (g < (size_t)N) {
            if (cnt[2][u]) atomicAdd(&gt_c[g], cnt[2][u]);
            if (cnt[3][u]) atomicAdd(&eq_c[g], cnt[3][u]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ statistics of one direction
constexpr int ST_MAXK = 16;
constexpr int ST_BINS = 4096;                      // 24-bit values: value >> 12, value & 4095
constexpr int ST_THREADS = 1024;
constexpr int ST_MAX_BLOCKS = 256;
constexpr unsigned ST_VMAX = (1u << 24) - 1;

struct KList {
    int k[ST_MAXK];
};

struct StatsHead {                                 // the front of the workspace
    unsigned long long hits[ST_MAXK];              // #{gt < K_t}
    unsigned long long sum;                        // Σ gt
    long long bin[2], before[2];                   // the high bin of the two middle ranks and the number of values below it
};

struct StatsLayout {
    size_t head, hi, lo, total;
};

StatsLayout stats_layout() {
    StatsLayout l;
    l.head = 0;
    l.hi = 256;                                    // unsigned [ST_BINS]
    l.lo = l.hi + ST_BINS * sizeof(unsigned);      // unsigned [2][ST_BINS]
    l.total = l.lo + 2 * ST_BINS * sizeof(unsigned);
    return l;
}
static_assert(sizeof(StatsHead) <= 256, "StatsHead outgrew its slot");

// a value outside [0, 2^24) cannot be a count of this build; it is clamped so that it stays inside the histograms
__device__ __forceinline__ unsigned st_value(int g) { return g < 0 ? 0u : ((unsigned)g > ST_VMAX ? ST_VMAX : (unsigned)g); }

__global__ __launch_bounds__(ST_THREADS) void st_count_kernel(int N, const int* __restrict__ gt, int nk, KList ks, StatsHead* __restrict__ head,
                                                              unsigned* __restrict__ hist_hi) {
    __shared__ unsigned hist[ST_BINS];
    __shared__ unsigned hits[ST_MAXK];
    __shared__ unsigned long long sum;
    const int tid = threadIdx.x;
    for (int i = tid; i < ST_BINS; i += ST_THREADS) hist[i] = 0;
    if (tid < ST_MAXK) hits[tid] = 0;
    if (tid == 0) sum = 0;
    __syncthreads();
    unsigned mine[ST_MAXK];
#pragma unroll
    for (int t = 0; t < ST_MAXK; ++t) mine[t] = 0;
    unsigned long long s = 0;
    for (size_t i = (size_t)blockIdx.x * ST_THREADS + tid; i < (size_t)N; i += (size_t)gridDim.x * ST_THREADS) {
        const unsigned v = st_value(gt[i]);
        s += v;
        atomicAdd(&hist[v >> 12], 1u);
#pragma unroll
        for (int t = 0; t < ST_MAXK; ++t) mine[t] += (t < nk && v < (unsigned)ks.k[t]) ? 1u : 0u;        // rank = 1 + gt <= K
    }
#pragma unroll
    for (int t = 0; t < ST_MAXK; ++t)
        if (mine[t]) atomicAdd(&hits[t], mine[t]);
    if (s) atomicAdd(&sum, s);
    __syncthreads();
    for (int i = tid; i < ST_BINS; i += ST_THREADS)
        if (hist[i]) atomicAdd(&hist_hi[i], hist[i]);
    if (tid < nk && hits[tid]) atomicAdd(&head->hits[tid], (unsigned long long)hits[tid]);
    if (tid == 0 && sum) atomicAdd(&head->sum, sum);
}

// The bin of `hist` (ST_BINS counters, thread t owns bins 4t .. 4t+3) that holds rank k (0-based), and the number of values in the bins below it.
__device__ void st_find_rank(const unsigned* __restrict__ hist, long long k, long long* scan, long long* bin, long long* before) {
    const int tid = threadIdx.x;
    constexpr int per = ST_BINS / ST_THREADS;
    if (tid == 0) {                                                // defined even if no thread finds k (k < the total is the caller's contract)
        *bin = 0;
        *before = 0;
    }
    unsigned c[per];
    long long own = 0;
#pragma unroll
    for (int i = 0; i < per; ++i) {
        c[i] = hist[tid * per + i];
        own += c[i];
    }
    scan[tid] = own;
    __syncthreads();
    for (int d = 1; d < ST_THREADS; d <<= 1) {                     // Hillis–Steele inclusive scan
        const long long o = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += o;
        __syncthreads();
    }
    long long acc = scan[tid] - own;
    if (acc <= k && k < scan[tid]) {
#pragma unroll
        for (int i = 0; i < per; ++i) {
            if (k >= acc && k < acc + c[i]) {
                *bin = tid * per + i;
                *before = acc;
            }
            acc += c[i];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(ST_THREADS) void st_pick_hi_kernel(int N, StatsHead* __restrict__ head, const unsigned* __restrict__ hist_hi) {
    __shared__ long long scan[ST_THREADS];
    __shared__ long long bin, before;
    for (int w = 0; w < 2; ++w) {                                  // the two middle ranks (the same one for odd N)
        st_find_rank(hist_hi, w == 0 ? (N - 1) / 2 : N / 2, scan, &bin, &before);
        if (threadIdx.x == 0) {
            head->bin[w] = bin;
            head->before[w] = before;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(ST_THREADS) void st_lo_kernel(int N, const int* __restrict__ gt, const StatsHead* __restrict__ head, unsigned* __restrict__ hist_lo) {
    __shared__ unsigned hist[2][ST_BINS];
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * ST_BINS; i += ST_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    const unsigned b0 = (unsigned)head->bin[0], b1 = (unsigned)head->bin[1];
    for (size_t i = (size_t)blockIdx.x * ST_THREADS + tid; i < (size_t)N; i += (size_t)gridDim.x * ST_THREADS) {
        const unsigned v = st_value(gt[i]);
        if ((v >> 12) == b0) atomicAdd(&hist[0][v & 4095], 1u);
        if ((v >> 12) == b1) atomicAdd(&hist[1][v & 4095], 1u);
    }
    __syncthreads();
    for (int i = tid; i < 2 * ST_BINS; i += ST_THREADS) {
        const unsigned h = (&hist[0][0])[i];
        if (h) atomicAdd(&hist_lo[i], h);
    }
}

__global__ __launch_bounds__(ST_THREADS) void st_final_kernel(int N, int nk, const StatsHead* __restrict__ head, const unsigned* __restrict__ hist_lo,
                                                              double* __restrict__ record) {
    __shared__ long long scan[ST_THREADS];
    __shared__ long long bin, before;
    long long mid[2];
    for (int w = 0; w < 2; ++w) {
        const long long k = (w == 0 ? (N - 1) / 2 : N / 2) - head->before[w];
        st_find_rank(hist_lo + w * ST_BINS, k, scan, &bin, &before);
        mid[w] = (head->bin[w] << 12) + bin;                       // gt of the middle query
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int t = 0; t < nk; ++t) record[t] = 100.0 * (double)head->hits[t] / (double)N;
        record[nk] = (double)(mid[0] + mid[1] + 2) * 0.5;          // ranks 1 + gt; exact: the sum is below 2^25
        record[nk + 1] = (double)(head->sum + (unsigned long long)N) / (double)N;      // Σ (1 + gt) is an integer below 2^49: one rounding, in the division
    }
}

// ------------------------------------------------------------------------------------------------ top-K listing
// One total order on the candidates (score, gallery index) of a query: score descending by IEEE comparison (+0 == -0), equal scores by index ascending;
// a NaN score is below every non-NaN score, NaN scores among themselves by index ascending.  An EMPTY list entry is (NaN, INT32_MAX): below every candidate.
constexpr int TK_MAXK = 32;
constexpr int TK_BLOCKS = 512;                     // the split rule aims at this many blocks: two per CU of a 256-CU device
constexpr int TK_LDS = RT_TILE / 2 + 1;            // row stride of the staged half tile of scores, in floats
constexpr int TK_EMPTY = 0x7fffffff;
constexpr size_t TK_STAGE_BYTES = 2 * RT_TILE * RT_LD * sizeof(float);
static_assert(RT_TILE * TK_LDS <= 2 * RT_TILE * RT_LD, "the staged half tile must fit into the operand stage");

// The order as one unsigned comparison: tk_ord is monotonic in the score (both zeros one value, NaN the lowest), the low word falls with the index.
// Only the comparisons use the key; the lists keep the score's own bits.
constexpr size_t TK_EXTRA_BYTES = (1 + 4) * RT_TILE * sizeof(unsigned);       // per row: the worst entry's tk_ord, four 32-column pass masks

__device__ __forceinline__ unsigned tk_ord(float s) {
    unsigned u = __builtin_bit_cast(unsigned, s);
    u = u == 0x80000000u ? 0u : u;                                 // -0 == +0
    const unsigned o = u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
    return s != s ? 0u : o;                                        // below -inf, whose value is 0x007fffff
}
__device__ __forceinline__ unsigned long long tk_key(float s, int i) { return ((unsigned long long)tk_ord(s) << 32) | (unsigned)~i; }
__device__ __forceinline__ bool tk_better(float s, int i, float t, int j) { return tk_key(s, i) > tk_key(t, j); }

struct TopkLayout {
    size_t an, bn, ps, pi, total;
    int max_splits;
};

int topk_rule(int Q, int N) {
    const int rt = (Q + RT_TILE - 1) / RT_TILE, ct = (N + RT_TILE - 1) / RT_TILE;
    const int want = rt >= TK_BLOCKS ? 1 : TK_BLOCKS / rt;
    return want < ct ? want : ct;
}

TopkLayout topk_layout(int Q, int N, int E, int K) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    TopkLayout l;
    l.max_splits = topk_rule(Q, N);                // an explicit split count is held to the rule's: the partial lists never outgrow TK_BLOCKS·128·K entries
    const size_t part = l.max_splits > 1 ? (size_t)l.max_splits * Q * K : 0;
    l.an = 0;                                      // float [Q][E]: normalised queries (normalize != 0 only)
    l.bn = up((size_t)Q * E * sizeof(float));      // float [N][E]: normalised gallery
    l.ps = l.bn + up((size_t)N * E * sizeof(float));       // float [splits][Q][K]: partial lists, scores
    l.pi = l.ps + up(part * sizeof(float));        // int   [splits][Q][K]: partial lists, gallery indices
    l.total = l.pi + up(part * sizeof(int));
    return l;
}

// Pass 1: block (x = row tile, y = split) owns 128 query rows and the gallery tiles [y·T/S, (y+1)·T/S) of the T column tiles.  Each tile's scores come from
// rt_tile_scores.  Selection in three steps per tile:
//   1. every lane tests its 64 accumulators against tk_ord of its rows' worst list entries (LDS, one word per row): score only, so a superset of what can
//      enter, and padding columns masked by index.  A wave ballot per (register, sub-tile) gives each row a 32-column pass mask, four masks per row.
//   2. the scores are staged half a tile at a time in the operand stage (free between two tiles);
//   3. thread r < 128 owns row r: it walks the set bits of the row's masks, tests each flagged score exactly against the row's worst entry (kept in
//      registers) and lets a winner take that entry's slot; K reads then find the new worst.  The list (LDS, [K][128]: entry j of every row side by side)
//      is therefore UNORDERED while it grows.  Once the lists are warm a tile flags a handful of scores, and the serial part is a few steps.
// The order is total, so the K entries after the last tile are the strip's first K whatever the tile order; they are written in order.
// Dynamic LDS: the operand stage, K·128 entries, 5·128 words of thresholds and masks.
static_assert(RT_TILE == 128, "the list epilogue splits its index with >> 7");
__global__ __launch_bounds__(RT_THREADS, 2) void tk_list_kernel(int Q, int N, int E, int K, const float* __restrict__ A, const float* __restrict__ B,
                                                             int* __restrict__ out_i, float* __restrict__ out_s) {
    extern __shared__ __attribute__((aligned(16))) float tk_smem[];
    float* As = tk_smem;
    float* Bs = tk_smem + RT_TILE * RT_LD;
    float* stage = tk_smem;                                        // aliases As / Bs: used only between two rt_tile_scores calls
    float* ls = tk_smem + 2 * RT_TILE * RT_LD;
    int* li = (int*)(ls + K * RT_TILE);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, c = lane & 31;
    const size_t m0 = (size_t)blockIdx.x * RT_TILE;
    const int ct = (N + RT_TILE - 1) / RT_TILE;
    const int t_begin = (int)((long long)blockIdx.y * ct / gridDim.y), t_end = (int)((long long)(blockIdx.y + 1) * ct / gridDim.y);
    const float nan = __builtin_nanf("");
    unsigned* tho = (unsigned*)(li + K * RT_TILE);                 // [128]: tk_ord of each row's worst entry (0 while the list has empty slots)
    unsigned* msk = tho + RT_TILE;                                 // [4][128]: word wn·2 + n of a row flags its columns wn·64 + n·32 + 0 .. 31
    for (int t = tid; t < K * RT_TILE; t += RT_THREADS) {
        ls[t] = nan;
        li[t] = TK_EMPTY;
    }
    if (tid < RT_TILE) tho[tid] = 0u;
    unsigned long long thr = tk_key(nan, TK_EMPTY);                // the row's worst entry and its slot (threads below 128, which own row tid)
    int thr_j = 0;
    const bool row_ok = tid < RT_TILE && m0 + tid < (size_t)Q;
    for (int tn = t_begin; tn < t_end; ++tn) {
        const size_t n0 = (size_t)tn * RT_TILE;
        f32x16 acc[2][2];
        rt_tile_scores(A, B, Q, N, E, m0, n0, As, Bs, acc);       // its barriers order the initialisation above before the first scan
        bool okj[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) okj[n] = n0 + (size_t)(wn * 64 + n * 32 + c) < (size_t)N;            // by index: padding is never selectable
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const unsigned t = tho[lr];
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const unsigned long long b = __ballot(okj[n] && tk_ord(acc[m][n][r]) >= t);
                    if (c == 0) msk[(wn * 2 + n) * RT_TILE + lr] = half ? (unsigned)(b >> 32) : (unsigned)b;
                }
            }
        for (int h = 0; h < 2; ++h) {
            if (wn == h) {
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                            stage[lr * TK_LDS + n * 32 + c] = acc[m][n][r];
                        }
            }
            __syncthreads();
            if (row_ok) {
                const int g0 = (int)n0 + h * (RT_TILE / 2);
                const float* row = stage + tid * TK_LDS;
                bool changed = false;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    unsigned mk = msk[(h * 2 + n) * RT_TILE + tid];
                    while (mk) {
                        const int cc = n * 32 + __builtin_ctz(mk);
                        mk &= mk - 1;
                        const float v = row[cc];
                        const int g = g0 + cc;
                        if (tk_key(v, g) <= thr) continue;
                        ls[thr_j * RT_TILE + tid] = v;                          // takes the worst entry's slot; then the new worst of the K
                        li[thr_j * RT_TILE + tid] = g;
                        changed = true;
                        thr = tk_key(ls[tid], li[tid]);
                        thr_j = 0;
#pragma unroll 4
                        for (int j = 1; j < K; ++j) {
                            const unsigned long long e = tk_key(ls[j * RT_TILE + tid], li[j * RT_TILE + tid]);
                            if (e < thr) {                                      // equal (empty) entries: the first stays the worst
                                thr = e;
                                thr_j = j;
                            }
                        }
                    }
                }
                if (changed) tho[tid] = (unsigned)(thr >> 32);
            }
            __syncthreads();                                       // the stage is free again: for the other half, then for the next tile's operands
        }
    }
    __syncthreads();                                               // a strip without tiles never met a barrier
    // The lists leave in order: entry j of row r goes to the place that the number of the row's entries before it gives (empty entries, all equal, keep
    // their slot order behind the candidates).  Row r is lane-contiguous in LDS, so every read below is conflict-free.
    const int rows = (size_t)Q - m0 < RT_TILE ? (int)((size_t)Q - m0) : RT_TILE;
    const size_t base = ((size_t)blockIdx.y * Q + m0) * K;        // [split][Q][K]; the one list [Q][K] when there is one split
    for (int t = tid; t < K * RT_TILE; t += RT_THREADS) {
        const int r = t & (RT_TILE - 1), j = t >> 7;
        if (r >= rows) continue;
        const float s = ls[t];
        const int i = li[t];
        int place = 0;
        for (int o = 0; o < K; ++o) {
            const float os = ls[o * RT_TILE + r];
            const int oi = li[o * RT_TILE + r];
            place += (tk_better(os, oi, s, i) || (oi == i && o < j)) ? 1 : 0;
        }
        out_s[base + (size_t)r * K + place] = s;
        out_i[base + (size_t)r * K + place] = i;
    }
}

// Pass 2: one wave per query row.  Place r of the result is the best of the row's S·K partial entries that comes strictly after place r - 1 in the order;
// candidates carry distinct gallery indices, so K rounds of a wave-wide minimum give the first K of the union.  (Empty entries are never reached: the
// strips together hold min(N, S·K) >= K candidates.)
__global__ __launch_bounds__(256) void tk_merge_kernel(int Q, int K, int S, const float* __restrict__ ps, const int* __restrict__ pi, int* __restrict__ idx,
                                                       float* __restrict__ score) {
    const size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= (size_t)Q) return;
    const int M = S * K;
    float prev_s = 0.f;
    int prev_i = -1;
    for (int r = 0; r < K; ++r) {
        float best_s = __builtin_nanf("");
        int best_i = TK_EMPTY;
        for (int e = lane; e < M; e += 64) {
            const int s = e / K, j = e - s * K;
            const size_t at = ((size_t)s * Q + q) * K + j;
            const float vs = ps[at];
            const int vi = pi[at];
            if ((r == 0 || tk_better(prev_s, prev_i, vs, vi)) && tk_better(vs, vi, best_s, best_i)) {
                best_s = vs;
                best_i = vi;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(best_s, o, 64);
            const int oi = __shfl_xor(best_i, o, 64);
            if (tk_better(os, oi, best_s, best_i)) {
                best_s = os;
                best_i = oi;
            }
        }
        if (lane == 0) {
            idx[q * K + r] = best_i;
            score[q * K + r] = best_s;
        }
        prev_s = best_s;
        prev_i = best_i;
    }
}

}  // namespace

size_t uia_retrieval_ranks_ws_bytes(int N, int E) {
    if (N < 1 || N > RT_MAXN || E < 4 || E > RT_MAXE || E % 4 != 0) return 0;
    return rank_layout(N, E).total;
}

int uia_retrieval_ranks_launch(hipStream_t stream, int N, int E, const float* img, const float* txt, int normalize, void* ws, size_t ws_bytes,
                               int32_t* gt_i2t, int32_t* eq_i2t, int32_t* gt_t2i, int32_t* eq_t2i) {
    UIA_CHECK_ARG(N >= 1 && N <= RT_MAXN && E >= 4 && E <= RT_MAXE && E % 4 == 0,
                  "uia_retrieval_ranks: bad shape N=%d E=%d (1 <= N <= %d, 4 <= E <= %d, E %% 4 == 0)", N, E, RT_MAXN, RT_MAXE);
    UIA_CHECK_ARG(img && txt && ws && gt_i2t && eq_i2t && gt_t2i && eq_t2i, "uia_retrieval_ranks: null tensor");
    UIA_CHECK_ARG(((uintptr_t)img | (uintptr_t)txt | (uintptr_t)ws) % 16 == 0, "uia_retrieval_ranks: img, txt and the workspace must be 16-byte aligned");
    const RankLayout l = rank_layout(N, E);
    UIA_CHECK_ARG(ws_bytes >= l.total, "uia_retrieval_ranks: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    char* base = (char*)ws;
    float* diag = (float*)(base + l.diag);
    const float* A = img;
    const float* B = txt;
    const size_t out_bytes = (size_t)N * sizeof(int32_t);
    UIA_CHECK_HIP(hipMemsetAsync(gt_i2t, 0, out_bytes, stream));
    UIA_CHECK_HIP(hipMemsetAsync(eq_i2t, 0, out_bytes, stream));
    UIA_CHECK_HIP(hipMemsetAsync(gt_t2i, 0, out_bytes, stream));
    UIA_CHECK_HIP(hipMemsetAsync(eq_t2i, 0, out_bytes, stream));
    UIA_CHECK_HIP(hipMemsetAsync(diag, 0, (size_t)N * sizeof(float), stream));
    if (normalize) {
        float* an = (float*)(base + l.an);
        float* bn = (float*)(base + l.bn);
        hipLaunchKernelGGL(rt_normalize_kernel, dim3((unsigned)((2 * (size_t)N + 3) / 4)), dim3(256), 0, stream, N, N, E, img, txt, an, bn);
        A = an;
        B = bn;
    }
    const int tiles = (N + RT_TILE - 1) / RT_TILE;
    hipLaunchKernelGGL(rt_diag_kernel, dim3((unsigned)tiles), dim3(RT_THREADS), 0, stream, N, E, A, B, diag);
    const int gy = tiles < RT_GRID_Y ? tiles : RT_GRID_Y;
    hipLaunchKernelGGL(rt_rank_kernel, dim3((unsigned)tiles, (unsigned)gy, (unsigned)((tiles + gy - 1) / gy)), dim3(RT_THREADS), 0, stream, N, E, A, B, diag,
                       gt_i2t, eq_i2t, gt_t2i, eq_t2i);
    UIA_CHECK_LAUNCH();
    return 0;
}

size_t uia_retrieval_stats_ws_bytes(int N) { return N >= 1 && N <= RT_MAXN ? stats_layout().total : 0; }

int uia_retrieval_stats_launch(hipStream_t stream, int N, const int32_t* gt, int nk, const int32_t* k_values, void* ws, size_t ws_bytes, double* record) {
    UIA_CHECK_ARG(N >= 1 && N <= RT_MAXN, "uia_retrieval_stats: bad size N=%d (1 <= N <= %d)", N, RT_MAXN);
    UIA_CHECK_ARG(nk >= 1 && nk <= ST_MAXK, "uia_retrieval_stats: bad count nk=%d of K values (1 <= nk <= %d)", nk, ST_MAXK);
    UIA_CHECK_ARG(gt && k_values && ws && record, "uia_retrieval_stats: null tensor");
    KList ks;
    for (int t = 0; t < ST_MAXK; ++t) ks.k[t] = t < nk ? k_values[t] : 1;
    for (int t = 0; t < nk; ++t) UIA_CHECK_ARG(ks.k[t] >= 1, "uia_retrieval_stats: bad K value k_values[%d]=%d (K >= 1)", t, ks.k[t]);
    const StatsLayout l = stats_layout();
    UIA_CHECK_ARG(ws_bytes >= l.total, "uia_retrieval_stats: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    char* base = (char*)ws;
    StatsHead* head = (StatsHead*)(base + l.head);
    unsigned* hist_hi = (unsigned*)(base + l.hi);
    unsigned* hist_lo = (unsigned*)(base + l.lo);
    const int want = (N + ST_THREADS - 1) / ST_THREADS;
    const int blocks = want < ST_MAX_BLOCKS ? want : ST_MAX_BLOCKS;
    UIA_CHECK_HIP(hipMemsetAsync(ws, 0, l.total, stream));
    hipLaunchKernelGGL(st_count_kernel, dim3(blocks), dim3(ST_THREADS), 0, stream, N, gt, nk, ks, head, hist_hi);
    hipLaunchKernelGGL(st_pick_hi_kernel, dim3(1), dim3(ST_THREADS), 0, stream, N, head, hist_hi);
    hipLaunchKernelGGL(st_lo_kernel, dim3(blocks), dim3(ST_THREADS), 0, stream, N, gt, head, hist_lo);
    hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(ST_THREADS), 0, stream, N, nk, head, hist_lo, record);
    UIA_CHECK_LAUNCH();
    return 0;
}

size_t uia_retrieval_topk_ws_bytes(int Q, int N, int E, int K) {
    if (Q < 1 || Q > RT_MAXN || N < 1 || N > RT_MAXN || E < 4 || E > RT_MAXE || E % 4 != 0 || K < 1 || K > TK_MAXK || K > N) return 0;
    return topk_layout(Q, N, E, K).total;
}

int uia_retrieval_topk_rule(int Q, int N) {
    if (Q < 1 || Q > RT_MAXN || N < 1 || N > RT_MAXN) return 1;
    return topk_rule(Q, N);
}

int uia_retrieval_topk_launch(hipStream_t stream, int Q, int N, int E, int K, const float* queries, const float* gallery, int normalize, int splits, void* ws,
                              size_t ws_bytes, int32_t* idx, float* score) {
    UIA_CHECK_ARG(Q >= 1 && Q <= RT_MAXN && N >= 1 && N <= RT_MAXN && E >= 4 && E <= RT_MAXE && E % 4 == 0,
                  "uia_retrieval_topk: bad shape Q=%d N=%d E=%d (1 <= Q, N <= %d, 4 <= E <= %d, E %% 4 == 0)", Q, N, E, RT_MAXN, RT_MAXE);
    UIA_CHECK_ARG(K >= 1 && K <= TK_MAXK && K <= N, "uia_retrieval_topk: bad K=%d (1 <= K <= min(N, %d), N=%d)", K, TK_MAXK, N);
    UIA_CHECK_ARG(queries && gallery && ws && idx && score, "uia_retrieval_topk: null tensor");
    UIA_CHECK_ARG(((uintptr_t)queries | (uintptr_t)gallery | (uintptr_t)ws) % 16 == 0,
                  "uia_retrieval_topk: queries, gallery and the workspace must be 16-byte aligned");
    UIA_CHECK_ARG(((uintptr_t)idx | (uintptr_t)score) % 4 == 0, "uia_retrieval_topk: idx and score must be 4-byte aligned");
    const TopkLayout l = topk_layout(Q, N, E, K);
    UIA_CHECK_ARG(splits >= 0 && splits <= TK_BLOCKS, "uia_retrieval_topk: bad splits=%d (0 = the rule, else 1 .. %d)", splits, TK_BLOCKS);
    UIA_CHECK_ARG(ws_bytes >= l.total, "uia_retrieval_topk: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
    const int S = splits == 0 || splits > l.max_splits ? l.max_splits : splits;        // never more strips than the rule's: that is what the workspace holds
    const size_t lds = TK_STAGE_BYTES + (size_t)K * RT_TILE * (sizeof(float) + sizeof(int)) + TK_EXTRA_BYTES;
    static UiaDevOnce once;                                        // K = 32 takes 69 120 B, past the 64 KiB a kernel gets unasked
    UIA_ENSURE_LDS_ATTR(once, tk_list_kernel, (int)(TK_STAGE_BYTES + (size_t)TK_MAXK * RT_TILE * (sizeof(float) + sizeof(int)) + TK_EXTRA_BYTES));
    char* base = (char*)ws;
    const float* A = queries;
    const float* B = gallery;
    if (normalize) {
        float* an = (float*)(base + l.an);
        float* bn = (float*)(base + l.bn);
        hipLaunchKernelGGL(rt_normalize_kernel, dim3((unsigned)(((size_t)Q + (size_t)N + 3) / 4)), dim3(256), 0, stream, Q, N, E, queries, gallery, an, bn);
        A = an;
        B = bn;
    }
    const int row_tiles = (Q + RT_TILE - 1) / RT_TILE;
    float* part_s = (float*)(base + l.ps);
    int* part_i = (int*)(base + l.pi);
    hipLaunchKernelGGL(tk_list_kernel, dim3((unsigned)row_tiles, (unsigned)S), dim3(RT_THREADS), lds, stream, Q, N, E, K, A, B, S == 1 ? idx : part_i,
                       S == 1 ? score : part_s);
    if (S > 1)
        hipLaunchKernelGGL(tk_merge_kernel, dim3((unsigned)(((size_t)Q + 3) / 4)), dim3(256), 0, stream, Q, K, S, part_s, part_i, idx, score);
    UIA_CHECK_LAUNCH();
    return 0;
}
