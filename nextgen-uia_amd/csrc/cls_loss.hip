// cls_loss.hip — the two device pieces of the supervised classification entry points (src/models/*/classification.py):
//   * uia_focal: MONAI FocalLoss(to_onehot_y=True) in its sigmoid form (gamma, optional alpha, mean over N·C), loss and d loss / d logits in one call;
//   * uia_binary_cls_stats: TP / FP / TN / FN at p1 > 0.5 and the tie-aware AUROC of a validation / test split (torchmetrics' binary task).
// Both are small row / vector kernels: no MFMA, wave64 reductions, fixed summation orders (no float atomics), so two calls on one input agree bit for bit.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int FOCAL_MAXC = 64;
constexpr int FOCAL_MAXN = 1 << 20;
constexpr int FOCAL_BLOCKS = 1024;          // upper bound of the first stage's grid = the workspace's partial sums
constexpr int STATS_THREADS = 1024;
constexpr int STATS_MAXN = 1 << 24;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Element e = n·C + c of the [N, C] logits, target t = (label[n] == c).  MONAI writes the element as
//   bce = x - x·t - logsigmoid(x),  loss = exp(γ·logsigmoid(-x·(2t-1))) · bce  (× t·α + (1-t)(1-α) with alpha).
// With z = t ? -x : x this is bce = softplus(z) and loss = sigmoid(z)^γ · softplus(z): the same function written without the cancellation of
// x - x·t - logsigmoid(x), every exp of a non-positive argument (logits of ±100 stay finite).  d loss / dz = sigmoid(z)^γ·(γ·sigmoid(-z)·softplus(z) + sigmoid(z)).
// A label outside [0, C) is never used as an index: it turns the row's loss and gradient into NaN.
__global__ __launch_bounds__(256) void focal_kernel(int N, int C, const float* __restrict__ logits, const int64_t* __restrict__ labels, float gamma,
                                                    float alpha, float inv_count, double* __restrict__ partial, float* __restrict__ dlogits) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t total = (size_t)N * C;
    double acc = 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + tid; e < total; e += (size_t)gridDim.x * 256) {
        const int n = (int)(e / C), c = (int)(e % C);
        const int64_t lab = labels[n];
        const bool t = lab == (int64_t)c;
        const bool bad = lab < 0 || lab >= (int64_t)C;
        const float x = logits[e];
        const float z = t ? -x : x;
        const float en = expf(-fabsf(z));
        const float l1p = log1pf(en);
        const float ls_z = fminf(z, 0.f) - l1p;             // logsigmoid(z)
        const float ls_mz = fminf(-z, 0.f) - l1p;           // logsigmoid(-z)
        const float sp = -ls_mz;                            // softplus(z) = bce
        const float w = expf(gamma * ls_z);                 // sigmoid(z)^γ
        const float at = alpha < 0.f ? 1.f : (t ? alpha : 1.f - alpha);
        float le = w * sp * at;
        float g = w * (gamma * expf(ls_mz) * sp + expf(ls_z)) * at * inv_count;
        g = t ? -g : g;
        if (bad) le = g = __builtin_nanf("");
        dlogits[e] = g;
        acc += (double)le;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// second stage: the first stage's partial sums in block order, one workgroup
__global__ __launch_bounds__(256) void focal_final_kernel(int nparts, const double* __restrict__ partial, double inv_count, float* __restrict__ loss) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nparts; i += 256) acc += partial[i];
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) *loss = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_count);
}

int focal_blocks(int N, int C) {
    const size_t g = ((size_t)N * C + 255) / 256;
    return (int)(g > FOCAL_BLOCKS ? FOCAL_BLOCKS : g);
}

// In-place inclusive scan of one value per thread over the workgroup (Hillis–Steele in LDS, STATS_THREADS entries of buf).
// op: 0 sum, 1 max, 2 min.  reverse: a suffix scan (thread t combines t..STATS_THREADS-1).
__device__ long long block_scan(long long v, long long* buf, int op, bool reverse) {
    const int tid = threadIdx.x;
    const int pos = reverse ? STATS_THREADS - 1 - tid : tid;
    buf[pos] = v;
    __syncthreads();
    for (int d = 1; d < STATS_THREADS; d <<= 1) {
        const bool has = pos >= d;
        const long long o = has ? buf[pos - d] : 0;
        __syncthreads();
        if (has) {
            long long cur = buf[pos];
            cur = op == 0 ? cur + o : (op == 1 ? (cur > o ? cur : o) : (cur < o ? cur : o));
            buf[pos] = cur;
        }
        __syncthreads();
    }
    const long long r = buf[pos];
    __syncthreads();
    return r;
}

// One workgroup.  Stage 0 (coalesced, strided over the threads): the counts at the threshold in input order, and the sorted scores / labels gathered
// once through perm into the workspace (s[k] = p1[perm[k]], y[k] = labels[perm[k]]), perm and the labels checked on the way.  Then thread t walks the
// sorted positions [t·chunk, (t+1)·chunk) of the staged arrays.  With P(k) = positives among sorted positions < k, a negative at k whose tie group
// spans [a, b] has P(a) positives strictly below and P(b+1) - P(a) tied with it; the Mann-Whitney count with ties at ½, doubled, is
//   Σ_neg (2·Npos - P(a) - P(b+1)),
// an integer: the AUROC is exact up to the final division.  P(a) of every position is a forward max-scan of P over the group starts, P(b+1) a backward
// min-scan over the group ends (P is non-decreasing); the scans run per thread over its chunk and across threads in LDS.
// rec: TP, FP, TN, FN, AUROC (fp64).  A label outside {0, 1} or a permutation entry outside [0, N) makes every field NaN.
__global__ __launch_bounds__(STATS_THREADS) void binary_stats_kernel(int N, const float* __restrict__ p1, const int64_t* __restrict__ labels,
                                                                     const int64_t* __restrict__ perm, void* ws, double* __restrict__ rec) {
    __shared__ long long buf[2 * STATS_THREADS];
    __shared__ long long tot[5];
    const int tid = threadIdx.x;
    float* ss = (float*)ws;                                 // sorted scores [N]
    unsigned char* ys = (unsigned char*)(ss + N);           // sorted labels [N]
    long long tp = 0, fp = 0, tn = 0, fn = 0, bad = 0;
    for (int i = tid; i < N; i += STATS_THREADS) {
        const int64_t y = labels[i];
        const bool pred = p1[i] > 0.5f;
        bad += (y != 0 && y != 1);
        tp += pred && y == 1;
        fp += pred && y == 0;
        tn += !pred && y == 0;
        fn += !pred && y == 1;
        const int64_t j = perm[i];
        const bool ok = j >= 0 && j < N;
        bad += !ok;
        ss[i] = ok ? p1[j] : 0.f;
        ys[i] = ok ? (unsigned char)(labels[j] == 1) : 0;
    }
    __syncthreads();                                        // the staged arrays are read by other threads of the workgroup below
    const int chunk = (N + STATS_THREADS - 1) / STATS_THREADS;
    const int k0 = tid * chunk < N ? tid * chunk : N, k1 = k0 + chunk < N ? k0 + chunk : N;
    // pass 1 over the sorted chunk: local positive count, P (local) at the last group start and at the first group end
    long long lp = 0, last_start = -1, first_end_next = -1;
    for (int k = k0; k < k1; ++k) {
        const float s = ss[k];
        if (k == 0 || s != ss[k - 1]) last_start = lp;
        lp += ys[k];
        if (first_end_next < 0 && (k == N - 1 || s != ss[k + 1])) first_end_next = lp;
    }
    const long long before = block_scan(lp, buf, 0, false) - lp;                                   // positives before the chunk
    const long long BIG = 1ll << 62;
    const long long carry_f = block_scan(last_start >= 0 ? before + last_start : -1, buf, 1, false);   // inclusive; exclusive part taken below
    const long long carry_b = block_scan(first_end_next >= 0 ? before + first_end_next : BIG, buf, 2, true);
    buf[tid] = carry_f;                                     // exclusive carries: the neighbouring thread's inclusive value
    buf[STATS_THREADS + tid] = carry_b;
    __syncthreads();
    long long pa = tid > 0 ? buf[tid - 1] : -1;
    long long pb = tid < STATS_THREADS - 1 ? buf[STATS_THREADS + tid + 1] : BIG;
    __syncthreads();
    // pass 2: Σ over the chunk's negatives of P(a) (forward) and P(b+1) (backward)
    long long sum_a = 0, sum_b = 0;
    lp = 0;
    for (int k = k0; k < k1; ++k) {
        if (k == 0 || ss[k] != ss[k - 1]) pa = before + lp;
        if (!ys[k]) sum_a += pa;
        lp += ys[k];
    }
    for (int k = k1 - 1; k >= k0; --k) {
        if (k == N - 1 || ss[k] != ss[k + 1]) pb = before + lp;
        lp -= ys[k];
        if (!ys[k]) sum_b += pb;
    }
    long long vals[5] = {tp, fp, tn, fn, bad};
    for (int i = 0; i < 5; ++i) {
        const long long v = block_scan(vals[i], buf, 0, false);
        if (tid == STATS_THREADS - 1) tot[i] = v;
    }
    const long long s = block_scan(sum_a + sum_b, buf, 0, false);
    __syncthreads();
    if (tid == STATS_THREADS - 1) {
        const long long npos = tot[0] + tot[3], nneg = tot[1] + tot[2];
        double auc = 0.0;                                   // one class absent: torchmetrics' ROC has an all-zero axis, area 0
        if (npos > 0 && nneg > 0) auc = (double)(2 * npos * nneg - s) / (2.0 * (double)npos * (double)nneg);
        const double nan = __builtin_nan("");
        const bool any_bad = tot[4] != 0;
        rec[0] = any_bad ? nan : (double)tot[0];
        rec[1] = any_bad ? nan : (double)tot[1];
        rec[2] = any_bad ? nan : (double)tot[2];
        rec[3] = any_bad ? nan : (double)tot[3];
        rec[4] = any_bad ? nan : auc;
    }
}

}  // namespace

size_t uia_focal_ws_bytes(int N, int C) {
    return (N > 0 && C > 0 ? (size_t)focal_blocks(N, C) : 1) * sizeof(double);
}

int uia_focal_launch(hipStream_t stream, int N, int C, const float* logits, const int64_t* labels, float gamma, float alpha, void* ws, size_t ws_bytes,
                     float* loss, float* dlogits) {
    UIA_CHECK_ARG(N >= 1 && N <= FOCAL_MAXN && C >= 2 && C <= FOCAL_MAXC, "uia_focal: bad shape N=%d C=%d (1 <= N <= %d, 2 <= C <= %d)", N, C, FOCAL_MAXN,
                  FOCAL_MAXC);
    UIA_CHECK_ARG(logits && labels && ws && loss && dlogits, "uia_focal: null tensor");
    UIA_CHECK_ARG(ws_bytes >= uia_focal_ws_bytes(N, C), "uia_focal: workspace of %zu bytes, %zu needed", ws_bytes, uia_focal_ws_bytes(N, C));
    UIA_CHECK_ARG(gamma >= 0.f && alpha <= 1.f, "uia_focal: gamma=%g must be >= 0 and alpha=%g <= 1 (negative: none)", (double)gamma, (double)alpha);
    const int g = focal_blocks(N, C);
    const double inv = 1.0 / ((double)N * C);
    hipLaunchKernelGGL(focal_kernel, dim3(g), dim3(256), 0, stream, N, C, logits, labels, gamma, alpha, (float)inv, (double*)ws, dlogits);
    hipLaunchKernelGGL(focal_final_kernel, dim3(1), dim3(256), 0, stream, g, (const double*)ws, inv, loss);
    UIA_CHECK_LAUNCH();
    return 0;
}

size_t uia_binary_cls_stats_ws_bytes(int N) { return (size_t)(N > 0 ? N : 0) * (sizeof(float) + 1); }       // the sorted scores and labels

int uia_binary_cls_stats_launch(hipStream_t stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes,
                                double* record) {
    UIA_CHECK_ARG(N >= 1 && N <= STATS_MAXN, "uia_binary_cls_stats: bad size N=%d (1 <= N <= %d)", N, STATS_MAXN);
    UIA_CHECK_ARG(p1 && labels && perm && ws && record, "uia_binary_cls_stats: null tensor");
    UIA_CHECK_ARG(ws_bytes >= uia_binary_cls_stats_ws_bytes(N), "uia_binary_cls_stats: workspace of %zu bytes, %zu needed", ws_bytes,
                  uia_binary_cls_stats_ws_bytes(N));
    hipLaunchKernelGGL(binary_stats_kernel, dim3(1), dim3(STATS_THREADS), 0, stream, N, p1, labels, perm, ws, record);
    UIA_CHECK_LAUNCH();
    return 0;
}
