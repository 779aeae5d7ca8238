// zero_shot.hip — the two device pieces of zero-shot classification (src/models/zero_shot_eval.py; the reference's src/models/*/zero_shot.py):
//   * uia_zero_shot_score: the prompt-ensemble scoring rule for one batch of image features, in one launch.  With f̂ = f / ||f|| for every image row and
//     every prompt row (no eps: the reference writes x / x.norm(), so a zero row is NaN),
//         s[i,t] = 100 · <f̂_img[i], f̂_prm[t]>,     logits[i,c] = (Σ_{t in class c, in prompt order} s[i,t]) / count_c      (fp32),
//     probs = softmax(logits) and, when asked, the normalised image rows themselves.
//   * uia_binary_roc_curve: the exact ROC curve of a split, torchmetrics ROC(task="binary", thresholds=None): point 0 is (0, 0, thr 1.0), then one point
//     per distinct score in descending order.
//
// Position independence (the contract of the scores): the bits of logits[i, :] depend only on row i of img and on the prompts, never on N, the batch or the
// place of the row in it.
//   - a row's norm is formed by ONE wave in a fixed order (lane-strided fmaf, the fixed butterfly of wave_sum), whichever block and wave gets the row;
//   - element k of a normalised row is the one correctly rounded quotient x[k] / norm, formed where the operand is staged;
//   - v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain from C = 0 (see retrieval.hip), every element of every tile runs it over k = 0 .. E-1,
//     and k past E is loaded as 0 for BOTH operands by index (fma(0, 0, acc) keeps acc);
//   - the class mean is a serial fp32 sum in prompt order (no contraction: __fmul_rn / __fadd_rn) and one division.
// An element of the product depends on one image row and one prompt row only, so a NaN row poisons exactly its own row (image) or column (prompt).
//
// Block: 32 image rows against every prompt column (T <= 256: at most eight 32-column tiles, padded by index), K step 32, four waves; wave w owns the
// column tiles w and w + 4.  Operands are staged [row][k] with a row stride of 33 floats: the one-float-per-lane fragment reads A[i = lane & 31][k = lane >> 5]
// are conflict-free, and so are the staging stores (a half-wave writes 32 consecutive k of one row).  C/D map: col = lane & 31,
// row = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5).  Epilogue: the scores go to LDS ([32][257], over the prompt stage), thread (row = tid & 31, c = tid >> 5)
// forms one logit, then thread row < 32 the row's softmax.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int ZS_MAXN = 1 << 24;
constexpr int ZS_MAXE = 4096;
constexpr int ZS_MAXC = 8;
constexpr int ZS_MAXP = 32;                        // prompts per class
constexpr int ZS_MAXT = 256;
constexpr int ZS_ROWS = 32;                        // image rows per block
constexpr int ZS_BK = 32;
constexpr int ZS_LD = ZS_BK + 1;                   // LDS row stride of the operand stages, in floats
constexpr int ZS_SLD = ZS_MAXT + 1;                // LDS row stride of the score tile
constexpr int ZS_THREADS = 256;
static_assert(ZS_ROWS * ZS_SLD <= ZS_MAXT * ZS_LD, "the score tile must fit into the prompt stage");
static_assert(ZS_ROWS * ZS_MAXC == ZS_THREADS, "one thread per (row, class) in the epilogue");

struct ClassOff {
    int off[ZS_MAXC + 1];
};

__global__ __launch_bounds__(ZS_THREADS) void zs_score_kernel(int N, int T, int E, int C, ClassOff co, const float* __restrict__ img,
                                                              const float* __restrict__ prompts, float* __restrict__ logits, long ld,
                                                              float* __restrict__ probs, float* __restrict__ img_n) {
    __shared__ float As[ZS_ROWS * ZS_LD];
    __shared__ float Bs[ZS_MAXT * ZS_LD];
    __shared__ float nrm_a[ZS_ROWS], nrm_b[ZS_MAXT];
    __shared__ float lg[ZS_ROWS][ZS_MAXC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t m0 = (size_t)blockIdx.x * ZS_ROWS;
    const int ntile = (T + 31) >> 5;

    // norms: one wave per row, the block's image rows first, then every prompt row (each block forms the prompt norms again: T·E reads, the size of the
    // prompt operand it reads anyway)
    for (int r = wave; r < ZS_ROWS + T; r += ZS_THREADS / 64) {
        const bool is_img = r < ZS_ROWS;
        const size_t gi = m0 + r;
        if (is_img && gi >= (size_t)N) continue;                  // wave-uniform; a padding row is masked by index below
        const float* src = is_img ? img + gi * E : prompts + (size_t)(r - ZS_ROWS) * E;
        float s = 0.f;
        for (int e = lane; e < E; e += 64) s = fmaf(src[e], src[e], s);
        const float nrm = sqrtf(wave_sum(s));
        if (lane == 0) (is_img ? nrm_a[r] : nrm_b[r - ZS_ROWS]) = nrm;
        if (is_img && img_n) {
            float* dst = img_n + gi * E;
            for (int e = lane; e < E; e += 64) dst[e] = src[e] / nrm;
        }
    }

    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const float* ap = As + (lane & 31) * ZS_LD + (lane >> 5);
    const float* bp = Bs + (wave * 32 + (lane & 31)) * ZS_LD + (lane >> 5);
    const bool has0 = wave < ntile, has1 = wave + 4 < ntile;      // wave-uniform
    for (int k0 = 0; k0 < E; k0 += ZS_BK) {
        __syncthreads();                                           // the norms are written / the previous step's fragment reads are done
        for (int idx = tid; idx < ZS_ROWS * ZS_BK; idx += ZS_THREADS) {
            const int r = idx >> 5, kk = idx & 31, k = k0 + kk;
            const size_t gi = m0 + r;
            As[r * ZS_LD + kk] = (gi < (size_t)N && k < E) ? img[gi * E + k] / nrm_a[r] : 0.f;
        }
        for (int idx = tid; idx < ntile * 32 * ZS_BK; idx += ZS_THREADS) {
            const int r = idx >> 5, kk = idx & 31, k = k0 + kk;
            Bs[r * ZS_LD + kk] = (r < T && k < E) ? prompts[(size_t)r * E + k] / nrm_b[r] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < ZS_BK / 2; ++kk) {
            const float a = ap[2 * kk];
            if (has0) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[2 * kk], acc[0], 0, 0, 0);
            if (has1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[128 * ZS_LD + 2 * kk], acc[1], 0, 0, 0);
        }
    }
    __syncthreads();                                               // the prompt stage is free: the score tile takes its place
    float* S = Bs;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        if (n == 0 ? has0 : has1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                S[row * ZS_SLD + (wave + 4 * n) * 32 + (lane & 31)] = acc[n][r];
            }
        }
    }
    __syncthreads();
    const int row = tid & 31, c = tid >> 5;
    const size_t gi = m0 + row;
    if (c < C) {
        const int t0 = co.off[c], t1 = co.off[c + 1];
        float sum = 0.f;
        for (int t = t0; t < t1; ++t) sum = __fadd_rn(sum, __fmul_rn(100.f, S[row * ZS_SLD + t]));
        const float v = sum / (float)(t1 - t0);
        lg[row][c] = v;
        if (gi < (size_t)N) logits[gi * ld + c] = v;
    }
    if (!probs) return;                                            // block-uniform
    __syncthreads();
    // softmax in its log-sum-exp form, in fp64: in fp32 the difference x - lse alone carries an error of half an ulp of |x| (4e-6 at 100), which is dozens of
    // ulps of the probability.  N·C values: the cost is nothing beside the product.
    if (tid < ZS_ROWS && gi < (size_t)N) {
        double m = (double)lg[tid][0];
        for (int j = 1; j < C; ++j) m = fmax(m, (double)lg[tid][j]);
        double z = 0.0;
        for (int j = 0; j < C; ++j) z += exp((double)lg[tid][j] - m);     // a NaN logit makes z, and with it the whole row, NaN
        const double lse = m + log(z);
        for (int j = 0; j < C; ++j) probs[gi * C + j] = (float)exp((double)lg[tid][j] - lse);
    }
}

// ------------------------------------------------------------------------------------------------ ROC curve
constexpr int ROC_THREADS = 1024;
constexpr int ROC_MAXN = 1 << 24;

// Inclusive sum scan of one value per thread over the workgroup (Hillis–Steele in LDS, ROC_THREADS entries of buf).
__device__ long long roc_scan(long long v, long long* buf) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < ROC_THREADS; d <<= 1) {
        const long long o = tid >= d ? buf[tid - d] : 0;
        __syncthreads();
        buf[tid] += o;
        __syncthreads();
    }
    const long long r = buf[tid];
    __syncthreads();
    return r;
}

// One workgroup, the scheme of binary_stats_kernel (cls_loss.hip).  Stage 0: the scores and labels gathered once through perm into the workspace in
// DESCENDING order (s[d] = p1[perm[N-1-d]]), labels, perm and scores checked on the way.  Thread t then owns the descending positions [t·chunk, (t+1)·chunk).
// Position d closes a tie group when d == N-1 or s[d] != s[d+1]; the group is one point of the curve: threshold s[d], TP = positives among positions <= d,
// FP = d + 1 - TP.  Its place in the output is 1 + the number of group ends before it: a scan of the per-thread counts, no atomics.  Both axes are ratios of
// integers, divided once in fp64; an absent class leaves its axis 0.
__global__ __launch_bounds__(ROC_THREADS) void roc_kernel(int N, const float* __restrict__ p1, const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ perm, void* ws, int32_t* __restrict__ count,
                                                          double* __restrict__ fpr, double* __restrict__ tpr, float* __restrict__ thr) {
    __shared__ long long buf[ROC_THREADS];
    __shared__ long long tot[3];
    const int tid = threadIdx.x;
    float* ss = (float*)ws;                                 // scores, descending [N]
    unsigned char* ys = (unsigned char*)(ss + N);           // their labels [N]
    long long bad = 0;
    for (int i = tid; i < N; i += ROC_THREADS) {
        const int64_t y = labels[i];
        const float p = p1[i];
        bad += (y != 0 && y != 1) || p != p;
        const int64_t j = perm[N - 1 - i];
        const bool ok = j >= 0 && j < N;
        bad += !ok;
        ss[i] = ok ? p1[j] : 0.f;
        ys[i] = ok ? (unsigned char)(labels[j] == 1) : 0;
    }
    __syncthreads();                                        // the staged arrays are read by other threads of the workgroup below
    const int chunk = (N + ROC_THREADS - 1) / ROC_THREADS;
    const int d0 = (long long)tid * chunk < N ? tid * chunk : N, d1 = d0 + chunk < N ? d0 + chunk : N;
    long long lp = 0, le = 0;                               // the chunk's positives and group ends
    for (int d = d0; d < d1; ++d) {
        lp += ys[d];
        le += (d == N - 1 || ss[d] != ss[d + 1]);
    }
    const long long vals[3] = {bad, lp, le};
    long long incl[3];
    for (int i = 0; i < 3; ++i) {
        incl[i] = roc_scan(vals[i], buf);
        if (tid == ROC_THREADS - 1) tot[i] = incl[i];
    }
    __syncthreads();
    if (tot[0] != 0) {                                      // workgroup-uniform
        if (tid == 0) *count = -1;
        return;
    }
    const long long npos = tot[1], nneg = (long long)N - npos;
    long long cp = incl[1] - lp, at = 1 + incl[2] - le;
    for (int d = d0; d < d1; ++d) {
        cp += ys[d];
        if (d == N - 1 || ss[d] != ss[d + 1]) {
            tpr[at] = npos > 0 ? (double)cp / (double)npos : 0.0;
            fpr[at] = nneg > 0 ? (double)((long long)d + 1 - cp) / (double)nneg : 0.0;
            thr[at] = ss[d];
            ++at;
        }
    }
    if (tid == 0) {
        fpr[0] = 0.0;
        tpr[0] = 0.0;
        thr[0] = 1.f;
        *count = (int32_t)(tot[2] + 1);
    }
}

}  // namespace

int uia_zero_shot_score_launch(hipStream_t stream, int N, int T, int E, int C, const int32_t* class_off, const float* img, const float* prompts, float* logits,
                               long ld, long row, float* probs, float* img_n) {
    UIA_CHECK_ARG(N >= 1 && N <= ZS_MAXN && E >= 1 && E <= ZS_MAXE, "uia_zero_shot_score: bad shape N=%d E=%d (1 <= N <= %d, 1 <= E <= %d)", N, E, ZS_MAXN,
                  ZS_MAXE);
    UIA_CHECK_ARG(C >= 2 && C <= ZS_MAXC, "uia_zero_shot_score: bad class count C=%d (2 <= C <= %d)", C, ZS_MAXC);
    UIA_CHECK_ARG(T >= 1 && T <= ZS_MAXT, "uia_zero_shot_score: bad prompt count T=%d (1 <= T <= %d)", T, ZS_MAXT);
    UIA_CHECK_ARG(class_off && img && prompts && logits, "uia_zero_shot_score: null tensor");
    UIA_CHECK_ARG(ld >= C && row >= 0, "uia_zero_shot_score: bad leading dimension ld=%ld (>= C=%d) or row offset %ld (>= 0)", ld, C, row);
    ClassOff co;
    for (int c = 0; c <= ZS_MAXC; ++c) co.off[c] = class_off[c < C ? c : C];
    UIA_CHECK_ARG(co.off[0] == 0 && co.off[C] == T, "uia_zero_shot_score: class_off must run from 0 to T=%d (got %d .. %d)", T, co.off[0], co.off[C]);
    for (int c = 0; c < C; ++c) {
        const long n = (long)co.off[c + 1] - (long)co.off[c];
        UIA_CHECK_ARG(n >= 1 && n <= ZS_MAXP, "uia_zero_shot_score: class %d has %ld prompts (1 <= prompts per class <= %d)", c, n, ZS_MAXP);
    }
    hipLaunchKernelGGL(zs_score_kernel, dim3((unsigned)((N + ZS_ROWS - 1) / ZS_ROWS)), dim3(ZS_THREADS), 0, stream, N, T, E, C, co, img, prompts,
                       logits + (size_t)row * (size_t)ld, ld, probs, img_n);
    UIA_CHECK_LAUNCH();
    return 0;
}

size_t uia_binary_roc_curve_ws_bytes(int N) { return (size_t)(N > 0 ? N : 0) * (sizeof(float) + 1); }       // the sorted scores and labels

int uia_binary_roc_curve_launch(hipStream_t stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes,
                                int32_t* count, double* fpr, double* tpr, float* thr) {
    UIA_CHECK_ARG(N >= 1 && N <= ROC_MAXN, "uia_binary_roc_curve: bad size N=%d (1 <= N <= %d)", N, ROC_MAXN);
    UIA_CHECK_ARG(p1 && labels && perm && ws && count && fpr && tpr && thr, "uia_binary_roc_curve: null tensor");
    UIA_CHECK_ARG(ws_bytes >= uia_binary_roc_curve_ws_bytes(N), "uia_binary_roc_curve: workspace of %zu bytes, %zu needed", ws_bytes,
                  uia_binary_roc_curve_ws_bytes(N));
    hipLaunchKernelGGL(roc_kernel, dim3(1), dim3(ROC_THREADS), 0, stream, N, p1, labels, perm, ws, count, fpr, tpr, thr);
    UIA_CHECK_LAUNCH();
    return 0;
}
