// components.hip — uia_mask_components: connected-component filtering of the native-size masks of uia_seg_predict_native (seg_native.hip) where they
// lie, in the one DEVICE byte buffer `buf`, plus one row per kept lesion.  Integers only; every result is exact and independent of scheduling.
//
// Per image b, HOST descriptor (mask_offset, H, W, overlay_offset or -1, min_area, keep, connectivity, 0): a mask byte != 0 is foreground; components are
// 4- or 8-connected; a component's first pixel is its smallest raster index y * W + x; components are ordered by (area descending, first pixel
// ascending); one is KEPT when area >= min_area and (keep == 0 or its position in that order < keep).  A pixel of a component that is not kept gets mask
// byte 0 and, with an overlay, green = red (the overlay is (g, max(g, p), g)); every other byte stays.  stats[b] = (foreground after, ymin, xmin, ymax,
// xmax after, components found, components kept, foreground before); list[b][k] = (area, ymin, xmin, ymax, xmax, first pixel, floor(sum y / area),
// floor(sum x / area)) of the k-th kept component, k < max_list <= 32, unused rows zero.
//
// The form: union-find on "label = image-local raster index of the root", merged with integer atomic-min, over plain launches on one stream.  Every phase
// that needs the one before it complete is its own launch; no workgroup ever waits for another.  A tile is 32 rows x 64 columns; workgroup k of a launch
// finds its image by a binary search in the prefix sums of the images' tile counts (1-D grid: a ragged batch wastes no workgroups).
//   scan      one workgroup: exclusive prefix sums of the images' pixel and tile counts (the label arrays lie back to back)
//   init      per image: the initial value of stats, the selection state, histograms, candidate rows
//   tile      a workgroup labels a tile wholly in LDS (union over the left / upper neighbours, then find), counts the tile-local roots' pixels in LDS
//             and writes label (int32 per pixel, -1 = background) and the partial area at the tile-local root (0 elsewhere)
//   seam      a thread per pixel on a tile's top row, left or right column unions it with its neighbours of smaller raster index in ANOTHER tile
//   flatten   every pixel finds its root and stores it; a tile-local root adds its partial area to the root's (one global atomic per tile and component)
//   select    radix select, 8 bits a round from the top, of the keep-th and of the min(keep, max_list)-th largest KEY = area << fbits | (fmask - first
//             pixel) per image: `hist` (roots matching the prefix so far count their digit: LDS per workgroup, then global atomics) and `pick` (per image:
//             the digit that holds the K-th largest) alternate, ceil(key bits / 8) rounds, key bits from the largest image of the batch.  Any keep works,
//             not only keep <= 32.  Skipped when no image has keep > 0 or max_list > 0 (min_area alone needs no ranking).
//   collect   roots at or above the list threshold append their key to the image's <= 32 candidate rows (which row is arbitrary; `final` ranks them)
//   rewrite   per pixel: root, area, key -> kept or not; bytes rewritten; stats and the listed components' boxes and coordinate sums accumulated per
//             thread over 8 pixels of a row, per workgroup in LDS, then with global integer atomics (sums in 64 bits)
//   final     per image: the candidates ranked by key, the list rows written, the unused rows zeroed
// Loops end by construction: labels obey label[p] <= p and only ever decrease, a find follows strictly decreasing labels, and a union retries only with
// the strictly smaller value an atomic-min returned.  In the seam pass other workgroups' labels change under a reader: labels are read with device-scope
// atomic loads, and any value a label ever held is a pixel of the same component with a smaller index, so an old value only lengthens a walk.  In the
// flatten pass the only stores are "label[p] = root of p": a reader sees p's former parent or its root, both on p's path, and a root's label never changes.
//
// Workspace: uia_mask_components_ws_bytes(B, pixels) = the sum, each term rounded up to 256 bytes, of
//   32 B (descriptor) + 4 (B + 1) + 4 (B + 1) (prefix sums) + 32 B (selection state) + 2048 B (histograms) + 4 B (candidate counts) + 256 B (candidate
//   keys) + 1024 B (candidate boxes and sums) + 4 pixels (labels) + 4 pixels (areas): 8 bytes per pixel and about 3.4 KiB per image.
// Bounds of the form (nothing was tuned beyond it): the LDS atomics of one address serialise (a full tile counts 2048 pixels into one word), and the
// select rounds each read every label again; see DESIGN.md §4 "Prediction: components".
#include <limits.h>

#include <algorithm>
#include <vector>

#include "uia_common.h"
#include "uia_kernels.h"

namespace {

typedef unsigned long long u64;

constexpr int MC_THREADS = 256;
constexpr int MC_TH = 32, MC_TW = 64, MC_TILE = MC_TH * MC_TW;     // a tile: 32 rows x 64 columns, 8 pixels per thread
constexpr int MC_SEAM = MC_TW + 2 * MC_TH;                         // seam candidates of a tile: its top row, left column and right column
constexpr int MC_DESC = 8, MC_MAX_B = 65535, MC_MAX_SIDE = 16384, MC_MAX_LIST = 32;
constexpr int MC_SCAN = 1024;

struct McSel {                 // one radix selection: the key's high bits decided so far (the threshold itself after the last round)
    u64 prefix;
    int k;                     // the K-th largest among the keys that match the prefix is wanted
    int active;                // 0: no selection (K == 0) or fewer than K components: the threshold is `prefix` as it stands
};
struct McAcc {                 // what the rewrite pass accumulates for a listed component
    int ymin, xmin, ymax, xmax;
    u64 sumy, sumx;
};
struct McWs {                  // the workspace's parts
    int32_t* desc;
    int32_t* pixbase;          // [B + 1]
    int32_t* tilebase;         // [B + 1]
    McSel* sel;                // [B][2]: 0 = the keep threshold, 1 = the list threshold
    int32_t* hist;             // [B][2][256]
    int32_t* ncand;            // [B]
    u64* candkey;              // [B][32]
    McAcc* acc;                // [B][32]
    int32_t* label;            // [pixels]
    int32_t* area;             // [pixels]
    size_t bytes;
};

inline size_t mc_up(size_t n) { return (n + 255) & ~(size_t)255; }

inline McWs mc_carve(void* ws, int B, int64_t pixels) {
    McWs w;
    uint8_t* p = (uint8_t*)ws;
    size_t at = 0;
    auto take = [&](size_t n) {
        uint8_t* r = p + at;
        at += mc_up(n);
        return r;
    };
    w.desc = (int32_t*)take((size_t)B * MC_DESC * 4);
    w.pixbase = (int32_t*)take((size_t)(B + 1) * 4);
    w.tilebase = (int32_t*)take((size_t)(B + 1) * 4);
    w.sel = (McSel*)take((size_t)B * 2 * sizeof(McSel));
    w.hist = (int32_t*)take((size_t)B * 2 * 256 * 4);
    w.ncand = (int32_t*)take((size_t)B * 4);
    w.candkey = (u64*)take((size_t)B * MC_MAX_LIST * 8);
    w.acc = (McAcc*)take((size_t)B * MC_MAX_LIST * sizeof(McAcc));
    w.label = (int32_t*)take((size_t)pixels * 4);
    w.area = (int32_t*)take((size_t)pixels * 4);
    w.bytes = at;
    return w;
}

__host__ __device__ inline int mc_tiles(int H, int W) { return ((H + MC_TH - 1) / MC_TH) * ((W + MC_TW - 1) / MC_TW); }

// ---------------------------------------------------------------- which image and which tile a workgroup has
struct McTile {
    int b, H, W, y0, x0, conn;
    size_t base;               // the image's first pixel in label / area
};
__device__ __forceinline__ McTile mc_locate(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase) {
    const int blk = blockIdx.x;
    int lo = 0, hi = B - 1;                        // the largest b with tilebase[b] <= blk: at most 16 halvings
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tilebase[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    McTile t;
    t.b = lo;
    const int32_t* d = desc + (size_t)lo * MC_DESC;
    t.H = d[1];
    t.W = d[2];
    t.conn = d[6];
    const int k = blk - tilebase[lo], tw = (t.W + MC_TW - 1) / MC_TW;
    t.y0 = (k / tw) * MC_TH;
    t.x0 = (k % tw) * MC_TW;
    t.base = (size_t)pixbase[lo];
    return t;
}

__device__ __forceinline__ u64 mc_key(int area, int first, int fbits) { return ((u64)(unsigned)area << fbits) | (u64)(((1u << fbits) - 1u) - (unsigned)first); }

// ---------------------------------------------------------------- scan and init
__global__ __launch_bounds__(MC_SCAN) void mc_scan_kernel(int B, const int32_t* __restrict__ desc, int32_t* __restrict__ pixbase, int32_t* __restrict__ tilebase) {
    __shared__ int sp[MC_SCAN], st[MC_SCAN];
    const int tid = threadIdx.x, chunk = (B + MC_SCAN - 1) / MC_SCAN;
    const int b0 = min(tid * chunk, B), b1 = min(b0 + chunk, B);
    int p = 0, t = 0;
    for (int b = b0; b < b1; ++b) {
        const int H = desc[(size_t)b * MC_DESC + 1], W = desc[(size_t)b * MC_DESC + 2];
        p += H * W;                                // the host checked: the batch's pixels are below 2^31
        t += mc_tiles(H, W);
    }
    sp[tid] = p;
    st[tid] = t;
    __syncthreads();
    for (int o = 1; o < MC_SCAN; o <<= 1) {        // inclusive scan over the threads' sums
        const int ap = tid >= o ? sp[tid - o] : 0, at = tid >= o ? st[tid - o] : 0;
        __syncthreads();
        sp[tid] += ap;
        st[tid] += at;
        __syncthreads();
    }
    p = sp[tid] - p;                               // exclusive
    t = st[tid] - t;
    for (int b = b0; b < b1; ++b) {
        const int H = desc[(size_t)b * MC_DESC + 1], W = desc[(size_t)b * MC_DESC + 2];
        pixbase[b] = p;
        tilebase[b] = t;
        p += H * W;
        t += mc_tiles(H, W);
    }
    if (tid == MC_SCAN - 1) {
        pixbase[B] = sp[tid];
        tilebase[B] = st[tid];
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_init_kernel(int max_list, const int32_t* __restrict__ desc, McSel* __restrict__ sel, int32_t* __restrict__ hist,
                                                             int32_t* __restrict__ ncand, u64* __restrict__ candkey, McAcc* __restrict__ acc, int32_t* __restrict__ stats) {
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    hist[b * 512 + tid] = 0;
    hist[b * 512 + 256 + tid] = 0;
    if (tid < MC_MAX_LIST) {
        candkey[b * MC_MAX_LIST + tid] = 0;
        McAcc a;
        a.ymin = a.xmin = INT_MAX;
        a.ymax = a.xmax = -1;
        a.sumy = a.sumx = 0;
        acc[b * MC_MAX_LIST + tid] = a;
    }
    if (tid < MC_DESC) stats[b * MC_DESC + tid] = (tid == 1 || tid == 2) ? INT_MAX : ((tid == 3 || tid == 4) ? -1 : 0);
    if (tid == 0) {
        const int keep = desc[b * MC_DESC + 5];
        const int rows = keep > 0 ? min(keep, max_list) : max_list;
        ncand[b] = 0;
        McSel s;
        s.prefix = 0;                              // threshold 0: every component is at or above it
        s.k = keep;
        s.active = keep > 0;
        sel[b * 2] = s;
        s.prefix = rows > 0 ? 0 : ~0ull;           // no list rows: no key reaches the threshold
        s.k = rows;
        s.active = rows > 0;
        sel[b * 2 + 1] = s;
    }
}

// ---------------------------------------------------------------- tile pass: union-find in LDS
__device__ __forceinline__ int mc_find_lds(volatile int* lab, int x) {
    int n;
    while ((n = lab[x]) != x) x = n;               // strictly decreasing: lab[x] <= x
    return x;
}
__device__ __forceinline__ void mc_union_lds(int* lab, int a, int b) {
    for (;;) {
        a = mc_find_lds(lab, a);
        b = mc_find_lds(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&lab[a], b);     // a > b: hang the larger root under the smaller
        if (old == a) return;                      // a was still a root
        a = old;                                   // old < a: somebody moved a meanwhile; go on from where it points
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_tile_kernel(int B, const uint8_t* __restrict__ buf, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                             const int32_t* __restrict__ tilebase, int32_t* __restrict__ label, int32_t* __restrict__ area) {
    __shared__ int lab[MC_TILE];
    __shared__ int cnt[MC_TILE];
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    const uint8_t* m = buf + (size_t)desc[(size_t)t.b * MC_DESC];
    const int tid = threadIdx.x;
    const bool eight = t.conn == 8;
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, y = t.y0 + i / MC_TW, x = t.x0 + i % MC_TW;
        const bool fg = y < t.H && x < t.W && m[(size_t)y * t.W + x] != 0;
        lab[i] = fg ? i : -1;
        cnt[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, ty = i / MC_TW, tx = i % MC_TW;
        if (lab[i] < 0) continue;
        if (tx > 0 && lab[i - 1] >= 0) mc_union_lds(lab, i, i - 1);
        if (ty > 0) {
            if (lab[i - MC_TW] >= 0) mc_union_lds(lab, i, i - MC_TW);
            if (eight) {
                if (tx > 0 && lab[i - MC_TW - 1] >= 0) mc_union_lds(lab, i, i - MC_TW - 1);
                if (tx < MC_TW - 1 && lab[i - MC_TW + 1] >= 0) mc_union_lds(lab, i, i - MC_TW + 1);
            }
        }
    }
    __syncthreads();
    int root[MC_TILE / MC_THREADS];
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS;
        root[k] = lab[i] < 0 ? -1 : mc_find_lds(lab, i);      // (nothing is stored between the barriers: the forest stands still)
    }
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k)
        if (root[k] >= 0) atomicAdd(&cnt[root[k]], 1);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, y = t.y0 + i / MC_TW, x = t.x0 + i % MC_TW;
        if (y >= t.H || x >= t.W) continue;
        const size_t at = t.base + (size_t)y * t.W + x;
        const int r = root[k];
        label[at] = r < 0 ? -1 : (t.y0 + r / MC_TW) * t.W + t.x0 + r % MC_TW;
        area[at] = r == i ? cnt[i] : 0;
    }
}

// ---------------------------------------------------------------- seam pass: union-find in global memory
__device__ __forceinline__ int mc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int mc_find_global(const int32_t* lab, int x) {
    int n;
    while ((n = mc_load(lab + x)) != x) x = n;     // strictly decreasing whatever age the value read has
    return x;
}
__device__ __forceinline__ void mc_union_global(int32_t* lab, int a, int b) {
    for (;;) {
        a = mc_find_global(lab, a);
        b = mc_find_global(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&lab[a], b);     // device scope; returns what memory held
        if (old == a) return;
        a = old;                                   // old < a
    }
}

__global__ __launch_bounds__(MC_SEAM) void mc_seam_kernel(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase,
                                                          int32_t* __restrict__ label) {
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    const int tid = threadIdx.x;
    int y, x;
    if (tid < MC_TW) {
        y = t.y0;
        x = t.x0 + tid;
    } else if (tid < MC_TW + MC_TH) {
        y = t.y0 + tid - MC_TW;
        x = t.x0;
    } else {
        y = t.y0 + tid - MC_TW - MC_TH;
        x = t.x0 + MC_TW - 1;
    }
    if (y >= t.H || x >= t.W) return;
    int32_t* lab = label + t.base;
    const int W = t.W, p = y * W + x;
    if (mc_load(lab + p) < 0) return;
    const bool eight = t.conn == 8;
    // the neighbours of smaller raster index that lie in another tile: the pixel of the pair with the larger index does the union
    const bool top = y == t.y0 && y > 0, left = x == t.x0 && x > 0, right = x == t.x0 + MC_TW - 1 && x + 1 < W;
    if (left && mc_load(lab + p - 1) >= 0) mc_union_global(lab, p, p - 1);
    if (top && mc_load(lab + p - W) >= 0) mc_union_global(lab, p, p - W);
    if (eight && y > 0) {
        if (x > 0 && (top || left) && mc_load(lab + p - W - 1) >= 0) mc_union_global(lab, p, p - W - 1);
        if (x + 1 < W && (top || right) && mc_load(lab + p - W + 1) >= 0) mc_union_global(lab, p, p - W + 1);
    }
}

// ---------------------------------------------------------------- flatten pass
__global__ __launch_bounds__(MC_THREADS) void mc_flatten_kernel(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase,
                                                                int32_t* label, int32_t* area) {
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    volatile int32_t* lab = label + t.base;
    int32_t* ar = area + t.base;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, y = t.y0 + i / MC_TW, x = t.x0 + i % MC_TW;
        if (y >= t.H || x >= t.W) continue;
        const int p = y * t.W + x;
        int r = lab[p];
        if (r < 0) continue;
        int n;
        while ((n = lab[r]) != r) r = n;
        lab[p] = r;
        const int part = ar[p];                    // > 0 only at a tile-local root; only roots of whole components are added to, and they skip this
        if (part > 0 && r != p) atomicAdd(&ar[r], part);
    }
}

// ---------------------------------------------------------------- selection
__global__ __launch_bounds__(MC_THREADS) void mc_hist_kernel(int B, int fbits, int shift, int first_round, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                             const int32_t* __restrict__ tilebase, const int32_t* __restrict__ label, const int32_t* __restrict__ area,
                                                             const McSel* __restrict__ sel, int32_t* __restrict__ hist) {
    __shared__ int h[2][256];
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    const McSel s0 = sel[(size_t)t.b * 2], s1 = sel[(size_t)t.b * 2 + 1];
    if (!s0.active && !s1.active) return;          // (uniform over the workgroup)
    const int tid = threadIdx.x;
    h[0][tid] = h[1][tid] = 0;
    __syncthreads();
    const int32_t* lab = label + t.base;
    const int32_t* ar = area + t.base;
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, y = t.y0 + i / MC_TW, x = t.x0 + i % MC_TW;
        if (y >= t.H || x >= t.W) continue;
        const int p = y * t.W + x;
        if (lab[p] != p) continue;                 // roots only
        const u64 key = mc_key(ar[p], p, fbits);
        const u64 high = first_round ? 0 : key >> (shift + 8);
        const int digit = (int)((key >> shift) & 255u);
        if (s0.active && high == s0.prefix) atomicAdd(&h[0][digit], 1);
        if (s1.active && high == s1.prefix) atomicAdd(&h[1][digit], 1);
    }
    __syncthreads();
    for (int s = 0; s < 2; ++s)
        if (h[s][tid]) atomicAdd(&hist[(size_t)t.b * 512 + s * 256 + tid], h[s][tid]);
}

__global__ __launch_bounds__(MC_THREADS) void mc_pick_kernel(McSel* __restrict__ sel, int32_t* __restrict__ hist) {
    __shared__ int h[2][256];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x;
    h[0][tid] = hist[b * 512 + tid];
    h[1][tid] = hist[b * 512 + 256 + tid];
    hist[b * 512 + tid] = 0;                       // ready for the next round
    hist[b * 512 + 256 + tid] = 0;
    __syncthreads();
    if (tid < 2) {
        McSel s = sel[b * 2 + tid];
        if (s.active) {
            int above = 0, d = 255;
            for (; d >= 0; --d) {                  // the largest digit with K <= the count of keys at or above it
                if (above + h[tid][d] >= s.k) break;
                above += h[tid][d];
            }
            if (d < 0) {                           // fewer than K components: all of them are at or above the threshold
                s.prefix = 0;
                s.active = 0;
            } else {
                s.prefix = (s.prefix << 8) | (u64)d;
                s.k -= above;
            }
            sel[b * 2 + tid] = s;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_collect_kernel(int B, int fbits, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                                const int32_t* __restrict__ tilebase, const int32_t* __restrict__ label, const int32_t* __restrict__ area,
                                                                const McSel* __restrict__ sel, int32_t* __restrict__ ncand, u64* __restrict__ candkey) {
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    const u64 tkeep = sel[(size_t)t.b * 2].prefix, tlist = sel[(size_t)t.b * 2 + 1].prefix;
    if (tlist == ~0ull) return;
    const int min_area = desc[(size_t)t.b * MC_DESC + 4];
    const int32_t* lab = label + t.base;
    const int32_t* ar = area + t.base;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < MC_TILE / MC_THREADS; ++k) {
        const int i = tid + k * MC_THREADS, y = t.y0 + i / MC_TW, x = t.x0 + i % MC_TW;
        if (y >= t.H || x >= t.W) continue;
        const int p = y * t.W + x;
        if (lab[p] != p) continue;
        const int a = ar[p];
        const u64 key = mc_key(a, p, fbits);
        if (a >= min_area && key >= tkeep && key >= tlist) {
            const int at = atomicAdd(&ncand[t.b], 1);          // keys are distinct, so at most K <= 32 of them reach the K-th largest
            if (at < MC_MAX_LIST) candkey[(size_t)t.b * MC_MAX_LIST + at] = key;
        }
    }
}

// ---------------------------------------------------------------- rewrite pass
__global__ __launch_bounds__(MC_THREADS) void mc_rewrite_kernel(int B, int fbits, uint8_t* __restrict__ buf, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                                const int32_t* __restrict__ tilebase, const int32_t* __restrict__ label, const int32_t* __restrict__ area,
                                                                const McSel* __restrict__ sel, const int32_t* __restrict__ ncand, const u64* __restrict__ candkey,
                                                                McAcc* __restrict__ acc, int32_t* __restrict__ stats) {
    __shared__ u64 ckey[MC_MAX_LIST];
    __shared__ int la[MC_MAX_LIST][6];             // ymin, xmin, ymax, xmax, sum y, sum x of this tile's share of a listed component
    __shared__ int st[8];
    const McTile t = mc_locate(B, desc, pixbase, tilebase);
    const int32_t* d = desc + (size_t)t.b * MC_DESC;
    uint8_t* m = buf + (size_t)d[0];
    uint8_t* ov = d[3] >= 0 ? buf + (size_t)d[3] : nullptr;
    const int min_area = d[4];
    const u64 tkeep = sel[(size_t)t.b * 2].prefix;
    const int nc = min(ncand[t.b], MC_MAX_LIST);
    const int tid = threadIdx.x;
    if (tid < MC_MAX_LIST) {
        ckey[tid] = tid < nc ? candkey[(size_t)t.b * MC_MAX_LIST + tid] : 0;
        la[tid][0] = la[tid][1] = INT_MAX;
        la[tid][2] = la[tid][3] = -1;
        la[tid][4] = la[tid][5] = 0;
    }
    if (tid < 8) st[tid] = (tid == 1 || tid == 2) ? INT_MAX : ((tid == 3 || tid == 4) ? -1 : 0);
    __syncthreads();

    const int32_t* lab = label + t.base;
    const int32_t* ar = area + t.base;
    const int y = t.y0 + tid / 8, xa = t.x0 + (tid % 8) * 8;   // a thread: 8 consecutive pixels of one row
    int after = 0, before = 0, found = 0, kept_n = 0, xmin = INT_MAX, xmax = -1;
    int last_r = -1, slot = -1;
    bool kept = false;
    int run_slot = -1, run_n = 0, run_x0 = 0, run_x1 = 0, run_sx = 0;
    auto flush = [&]() {
        if (run_slot >= 0) {
            atomicMin(&la[run_slot][0], y);
            atomicMin(&la[run_slot][1], run_x0);
            atomicMax(&la[run_slot][2], y);
            atomicMax(&la[run_slot][3], run_x1);
            atomicAdd(&la[run_slot][4], y * run_n);            // a tile's share: at most 2048 * 16383 < 2^31
            atomicAdd(&la[run_slot][5], run_sx);
        }
        run_slot = -1;
    };
    if (y < t.H) {
        for (int e = 0; e < 8; ++e) {
            const int x = xa + e;
            if (x >= t.W) break;
            const int p = y * t.W + x, r = lab[p];
            if (r < 0) continue;
            if (r != last_r) {
                last_r = r;
                const int a = ar[r];
                const u64 key = mc_key(a, r, fbits);
                kept = a >= min_area && key >= tkeep;
                slot = -1;
                if (kept)
                    for (int c = 0; c < nc; ++c)
                        if (ckey[c] == key) slot = c;
            }
            ++before;
            if (r == p) {
                ++found;
                kept_n += kept;
            }
            if (kept) {
                ++after;
                xmin = min(xmin, x);
                xmax = max(xmax, x);
                if (slot >= 0) {
                    if (slot != run_slot) {
                        flush();
                        run_slot = slot;
                        run_n = 0;
                        run_x0 = x;
                        run_sx = 0;
                    }
                    ++run_n;
                    run_x1 = x;
                    run_sx += x;
                }
            } else {
                m[p] = 0;
                if (ov) ov[3 * (size_t)p + 1] = ov[3 * (size_t)p];
            }
        }
        flush();
    }
    if (before) {
        atomicAdd(&st[7], before);
        if (found) atomicAdd(&st[5], found);
        if (kept_n) atomicAdd(&st[6], kept_n);
        if (after) {
            atomicAdd(&st[0], after);
            atomicMin(&st[1], y);
            atomicMin(&st[2], xmin);
            atomicMax(&st[3], y);
            atomicMax(&st[4], xmax);
        }
    }
    __syncthreads();
    if (tid < 8 && st[7]) {
        int32_t* s = stats + (size_t)t.b * MC_DESC;
        const int v = st[tid];
        if (tid == 1 || tid == 2) {
            if (v != INT_MAX) atomicMin(&s[tid], v);
        } else if (tid == 3 || tid == 4) {
            if (v >= 0) atomicMax(&s[tid], v);
        } else if (v) {
            atomicAdd(&s[tid], v);
        }
    }
    if (tid >= 32 && tid < 32 + MC_MAX_LIST) {
        const int c = tid - 32;
        if (c < nc && la[c][2] >= 0) {
            McAcc* a = acc + (size_t)t.b * MC_MAX_LIST + c;
            atomicMin(&a->ymin, la[c][0]);
            atomicMin(&a->xmin, la[c][1]);
            atomicMax(&a->ymax, la[c][2]);
            atomicMax(&a->xmax, la[c][3]);
            atomicAdd(&a->sumy, (u64)la[c][4]);
            atomicAdd(&a->sumx, (u64)la[c][5]);
        }
    }
}

__global__ __launch_bounds__(64) void mc_final_kernel(int fbits, int max_list, const int32_t* __restrict__ ncand, const u64* __restrict__ candkey, const McAcc* __restrict__ acc,
                                                      int32_t* __restrict__ list) {
    __shared__ u64 ckey[MC_MAX_LIST];
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, nc = min(ncand[b], MC_MAX_LIST);
    if (tid < MC_MAX_LIST) ckey[tid] = tid < nc ? candkey[b * MC_MAX_LIST + tid] : 0;
    __syncthreads();
    if (tid < nc) {
        const u64 key = ckey[tid];
        int rank = 0;
        for (int c = 0; c < nc; ++c) rank += ckey[c] > key;    // keys are distinct: the ranks are 0 .. nc - 1
        if (rank < max_list) {
            const McAcc a = acc[b * MC_MAX_LIST + tid];
            const u64 ar = key >> fbits;
            int32_t* row = list + (b * max_list + rank) * 8;
            row[0] = (int)ar;
            row[1] = a.ymin;
            row[2] = a.xmin;
            row[3] = a.ymax;
            row[4] = a.xmax;
            row[5] = (int)(((1u << fbits) - 1u) - (unsigned)(key & ((1ull << fbits) - 1ull)));
            row[6] = (int)(a.sumy / ar);
            row[7] = (int)(a.sumx / ar);
        }
    }
    if (tid >= 32) {
        const int k = tid - 32;
        if (k >= nc && k < max_list)
            for (int w = 0; w < 8; ++w) list[(b * max_list + k) * 8 + w] = 0;
    }
}

struct Range {
    uintptr_t lo, hi;
    int image;
    bool overlay;
};

inline int mc_bits(unsigned long long v) {
    int n = 0;
    while (v) {
        ++n;
        v >>= 1;
    }
    return n;
}

}  // namespace

size_t uia_mask_components_ws_bytes(int B, int64_t pixels) {
    if (B < 1 || B > MC_MAX_B || pixels < 1 || pixels > 0x7fffffffLL) return 0;
    return mc_carve(nullptr, B, pixels).bytes;
}

int uia_mask_components_launch(hipStream_t stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats, int32_t* list,
                               int max_list) {
    const char* who = "uia_mask_components";
    UIA_CHECK_ARG(B >= 1 && B <= MC_MAX_B, "%s: bad shape B=%d (1 <= B <= %d)", who, B, MC_MAX_B);
    UIA_CHECK_ARG(max_list >= 0 && max_list <= MC_MAX_LIST, "%s: max_list=%d (0 .. %d)", who, max_list, MC_MAX_LIST);
    UIA_CHECK_ARG(buf && desc && ws && stats, "%s: null tensor (buf, desc, ws and stats are required)", who);
    UIA_CHECK_ARG(list || max_list == 0, "%s: null list with max_list=%d", who, max_list);
    UIA_CHECK_ARG(buf_bytes >= 1 && buf_bytes <= 0x7fffffffu, "%s: a buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, buf_bytes);
    UIA_CHECK_ARG((uintptr_t)ws % 8 == 0 && (uintptr_t)stats % 4 == 0 && (uintptr_t)list % 4 == 0, "%s: the workspace must be 8-byte, stats and list 4-byte aligned", who);
    std::vector<Range> ranges;
    ranges.reserve(2 * (size_t)B);
    unsigned long long pixels = 0, tiles = 0, largest = 1;
    bool ranking = max_list > 0;
    for (int b = 0; b < B; ++b) {                                  // every image is checked before anything is enqueued
        const int32_t* d = desc + (size_t)b * MC_DESC;
        const long long moff = d[0], H = d[1], W = d[2], ooff = d[3], min_area = d[4], keep = d[5], conn = d[6];
        UIA_CHECK_ARG(d[7] == 0, "%s: image %d has a non-zero reserved descriptor word (%d)", who, b, d[7]);
        UIA_CHECK_ARG(H >= 1 && W >= 1 && H <= MC_MAX_SIDE && W <= MC_MAX_SIDE, "%s: image %d is %lld x %lld (1 .. %d a side)", who, b, H, W, MC_MAX_SIDE);
        UIA_CHECK_ARG(conn == 4 || conn == 8, "%s: image %d has connectivity %lld (4 or 8)", who, b, conn);
        UIA_CHECK_ARG(min_area >= 0 && keep >= 0, "%s: image %d has min_area %lld and keep %lld (neither may be negative)", who, b, min_area, keep);
        UIA_CHECK_ARG(ooff >= -1, "%s: image %d has overlay offset %lld (an offset, or -1 for none)", who, b, ooff);
        const unsigned long long px = (unsigned long long)H * W;
        UIA_CHECK_ARG(moff >= 0 && (unsigned long long)moff + px <= buf_bytes, "%s: the mask of image %d (offset %lld, %lld x %lld) leaves the buffer of %zu bytes", who, b, moff,
                      H, W, buf_bytes);
        ranges.push_back({(uintptr_t)buf + (uintptr_t)moff, (uintptr_t)buf + (uintptr_t)moff + (uintptr_t)px, b, false});
        if (ooff >= 0) {
            UIA_CHECK_ARG((unsigned long long)ooff + 3 * px <= buf_bytes, "%s: the overlay of image %d (offset %lld, %lld x %lld x 3) leaves the buffer of %zu bytes", who, b,
                          ooff, H, W, buf_bytes);
            ranges.push_back({(uintptr_t)buf + (uintptr_t)ooff, (uintptr_t)buf + (uintptr_t)ooff + (uintptr_t)(3 * px), b, true});
        }
        pixels += px;
        tiles += (unsigned long long)mc_tiles((int)H, (int)W);
        largest = std::max(largest, px);
        ranking = ranking || keep > 0;
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.image < b.image; });
    for (size_t i = 1; i < ranges.size(); ++i)                     // sorted by start: two ranges overlap iff some neighbours do
        UIA_CHECK_ARG(ranges[i - 1].hi <= ranges[i].lo, "%s: the %s of image %d overlaps the %s of image %d", who, ranges[i - 1].overlay ? "overlay" : "mask",
                      ranges[i - 1].image, ranges[i].overlay ? "overlay" : "mask", ranges[i].image);
    // the masks are disjoint parts of a buffer below 2^31 bytes, so the batch's pixels are below 2^31 as well
    const size_t need = uia_mask_components_ws_bytes(B, (int64_t)pixels);
    UIA_CHECK_ARG(need != 0 && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    struct Fixed {
        uintptr_t lo, hi;
        const char* name;
    };
    const Fixed fixed[3] = {{(uintptr_t)stats, (uintptr_t)stats + (size_t)B * MC_DESC * sizeof(int32_t), "stats"},
                            {max_list ? (uintptr_t)list : 0, max_list ? (uintptr_t)list + (size_t)B * max_list * 8 * sizeof(int32_t) : 0, "list"},
                            {(uintptr_t)ws, (uintptr_t)ws + need, "the workspace"}};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            UIA_CHECK_ARG(!(fixed[i].lo < fixed[j].hi && fixed[j].lo < fixed[i].hi), "%s: %s overlaps %s", who, fixed[i].name, fixed[j].name);
    for (const Range& r : ranges)
        for (int i = 0; i < 3; ++i)
            UIA_CHECK_ARG(!(r.lo < fixed[i].hi && fixed[i].lo < r.hi), "%s: the %s of image %d overlaps %s", who, r.overlay ? "overlay" : "mask", r.image, fixed[i].name);

    const McWs w = mc_carve(ws, B, (int64_t)pixels);
    const int fbits = mc_bits(largest - 1), rounds = (fbits + mc_bits(largest) + 7) / 8;       // key = area << fbits | (2^fbits - 1 - first pixel)
    const dim3 grid((unsigned)tiles), block(MC_THREADS);
    UIA_CHECK_HIP(hipMemcpyAsync(w.desc, desc, (size_t)B * MC_DESC * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    mc_scan_kernel<<<dim3(1), dim3(MC_SCAN), 0, stream>>>(B, w.desc, w.pixbase, w.tilebase);
    UIA_CHECK_LAUNCH();
    mc_init_kernel<<<dim3((unsigned)B), block, 0, stream>>>(max_list, w.desc, w.sel, w.hist, w.ncand, w.candkey, w.acc, stats);
    UIA_CHECK_LAUNCH();
    mc_tile_kernel<<<grid, block, 0, stream>>>(B, buf, w.desc, w.pixbase, w.tilebase, w.label, w.area);
    UIA_CHECK_LAUNCH();
    if (tiles > (unsigned long long)B) {                           // some image has more than one tile
        mc_seam_kernel<<<grid, dim3(MC_SEAM), 0, stream>>>(B, w.desc, w.pixbase, w.tilebase, w.label);
        UIA_CHECK_LAUNCH();
    }
    mc_flatten_kernel<<<grid, block, 0, stream>>>(B, w.desc, w.pixbase, w.tilebase, w.label, w.area);
    UIA_CHECK_LAUNCH();
    if (ranking) {
        for (int r = 0; r < rounds; ++r) {
            mc_hist_kernel<<<grid, block, 0, stream>>>(B, fbits, 8 * (rounds - 1 - r), r == 0, w.desc, w.pixbase, w.tilebase, w.label, w.area, w.sel, w.hist);
            UIA_CHECK_LAUNCH();
            mc_pick_kernel<<<dim3((unsigned)B), block, 0, stream>>>(w.sel, w.hist);
            UIA_CHECK_LAUNCH();
        }
        if (max_list > 0) {
            mc_collect_kernel<<<grid, block, 0, stream>>>(B, fbits, w.desc, w.pixbase, w.tilebase, w.label, w.area, w.sel, w.ncand, w.candkey);
            UIA_CHECK_LAUNCH();
        }
    }
    mc_rewrite_kernel<<<grid, block, 0, stream>>>(B, fbits, buf, w.desc, w.pixbase, w.tilebase, w.label, w.area, w.sel, w.ncand, w.candkey, w.acc, stats);
    UIA_CHECK_LAUNCH();
    if (max_list > 0) {
        mc_final_kernel<<<dim3((unsigned)B), dim3(64), 0, stream>>>(fbits, max_list, w.ncand, w.candkey, w.acc, list);
        UIA_CHECK_LAUNCH();
    }
    return 0;
}
