// morphology.hip — uia_mask_morphology: disk closing, hole filling and disk opening of the native-size masks of uia_seg_predict_native (seg_native.hip)
// where they lie, in the one DEVICE byte buffer `buf`, before uia_mask_components (components.hip) ranks what is left.  Integers only; every result is
// exact and independent of scheduling.
//
// Per image b, HOST descriptor (mask_offset, H, W, overlay_offset or -1, r_close, r_open, hole_area, hole_connectivity): a mask byte != 0 is foreground;
// D is the image's pixel grid, disk(r) = {(dy, dx) : dy^2 + dx^2 <= r^2};  dilate_r(X) = {p in D : some q in X with p - q in disk(r)} (pixels outside the
// image contribute nothing);  erode_r(X) = D \ dilate_r(D \ X) (only background INSIDE the image erodes);  a hole is a connected component of the
// background, 4- or 8-connected per hole_connectivity, with no pixel in the first or last row or column; it is filled when hole_area == -1 or its area <=
// hole_area (0: no fill).  X1 = erode_rc(dilate_rc(X0)), X2 = X1 + the filled holes of X1, X3 = dilate_ro(erode_ro(X2)); a radius of 0 is the identity.
// A pixel of X3 \ X0 gets mask byte 255 and, with an overlay, green = 255; a pixel of X0 \ X3 gets 0 and green = red; every other byte stays.
// stats[b] = (foreground after, ymin, xmin, ymax, xmax after, pixels added, pixels removed, foreground before).
//
// The form: plain launches on one stream; every phase that needs the one before it complete is its own launch, and no workgroup ever waits for another.
// A tile is 32 rows x 64 columns (components.hip's, so that the fill and the passes share one tile count); workgroup k of a launch finds its image by a
// binary search in the prefix sums of the images' tile counts.  An image's set travels through two byte planes of the workspace (0 / 1 per pixel): phase
// number n of an image reads the mask itself (n = 0), plane A (n odd) or plane B (n even) and writes the other plane, so an image that skips a phase (its
// radius is 0, its hole_area is 0) costs nothing but a workgroup that returns.
//   scan      one workgroup: exclusive prefix sums of the images' pixel and tile counts; the initial value of stats
//   pass      dilation-type pass of radius r <= 64 (dilate: of the set; erode: of the in-image complement, the result inverted).  A workgroup takes its
//             tile plus a halo of r pixels a side into LDS as bytes "set / not set" ((32 + 2r) x (64 + 2r) <= 30 KiB), turns every column in place into
//             g = the vertical distance to the nearest set pixel, capped at r + 1 (one sweep down, one up; a thread per column), and then decides every
//             pixel of the tile: it is within r of the set iff g(y, x + dx)^2 + dx^2 <= r^2 for some |dx| <= r; the scan stops at the first hit.  Exact.
//   tile / seam / flatten    components.hip's union-find ("label = image-local raster index of the root", integer atomic-min), a self-contained copy run
//             on the BACKGROUND of the current plane; the area word of a root also carries a flag "touches the image's frame" (bit 30; areas are < 2^29)
//   fill      per pixel: foreground, or background whose root has no frame flag and an area within hole_area -> the next plane
//   final     per pixel: the last plane against the mask: changed bytes rewritten with byte stores, the overlay's green byte with them; stats folded per
//             thread, per workgroup in LDS, then with global integer atomics
// Loops end by construction: the sweeps and the dx scan are counted; the union-find is components.hip's (labels obey label[p] <= p and only ever
// decrease, a find follows strictly decreasing labels, a union retries only with the strictly smaller value an atomic-min returned).
//
// Workspace: uia_mask_morphology_ws_bytes(B, pixels) = the sum, each term rounded up to 256 bytes, of 32 B (descriptor) + 4 (B + 1) + 4 (B + 1) (prefix
// sums) + pixels + pixels (the two planes) + 4 pixels (labels) + 4 pixels (areas): 10 bytes per pixel and about 40 bytes per image.
#include <limits.h>

#include <algorithm>
#include <vector>

#include "uia_common.h"
#include "uia_kernels.h"

namespace {

constexpr int MM_THREADS = 256;
constexpr int MM_TH = 32, MM_TW = 64, MM_TILE = MM_TH * MM_TW;     // a tile: 32 rows x 64 columns, 8 pixels per thread
constexpr int MM_SEAM = MM_TW + 2 * MM_TH;
constexpr int MM_DESC = 8, MM_MAX_B = 65535, MM_MAX_SIDE = 16384, MM_MAX_R = 64;
constexpr int MM_SCAN = 1024;
constexpr int MM_FRAME = 1 << 30, MM_AREA = MM_FRAME - 1;          // the area word of a background root: the frame flag and the pixel count
// the phases of an image, in order; an image's n-th ACTIVE phase reads plane (n odd ? A : B), or the mask at n = 0, and writes the other plane
enum { MM_DILATE_C = 0, MM_ERODE_C = 1, MM_FILL = 2, MM_ERODE_O = 3, MM_DILATE_O = 4, MM_FINAL = 5 };

struct MmWs {
    int32_t* desc;
    int32_t* pixbase;          // [B + 1]
    int32_t* tilebase;         // [B + 1]
    uint8_t* plane[2];         // [pixels] each
    int32_t* label;            // [pixels]
    int32_t* area;             // [pixels]
    size_t bytes;
};

inline size_t mm_up(size_t n) { return (n + 255) & ~(size_t)255; }

inline MmWs mm_carve(void* ws, int B, int64_t pixels) {
    MmWs w;
    uint8_t* p = (uint8_t*)ws;
    size_t at = 0;
    auto take = [&](size_t n) {
        uint8_t* r = p + at;
        at += mm_up(n);
        return r;
    };
    w.desc = (int32_t*)take((size_t)B * MM_DESC * 4);
    w.pixbase = (int32_t*)take((size_t)(B + 1) * 4);
    w.tilebase = (int32_t*)take((size_t)(B + 1) * 4);
    w.plane[0] = take((size_t)pixels);
    w.plane[1] = take((size_t)pixels);
    w.label = (int32_t*)take((size_t)pixels * 4);
    w.area = (int32_t*)take((size_t)pixels * 4);
    w.bytes = at;
    return w;
}

__host__ __device__ inline int mm_tiles(int H, int W) { return ((H + MM_TH - 1) / MM_TH) * ((W + MM_TW - 1) / MM_TW); }

// the number of active phases of an image before phase `phase`
__host__ __device__ inline int mm_before(const int32_t* d, int phase) {
    int n = 0;
    if (d[4] > 0) n += phase < 2 ? phase : 2;
    if (d[6] != 0 && phase > MM_FILL) n += 1;
    if (d[5] > 0 && phase > MM_ERODE_O) n += phase - MM_ERODE_O;       // (phase <= MM_FINAL: at most 2)
    return n;
}

// ---------------------------------------------------------------- which image and which tile a workgroup has
struct MmTile {
    int b, H, W, y0, x0;
    size_t base;               // the image's first pixel in the planes, label and area
    const int32_t* d;
};
__device__ __forceinline__ MmTile mm_locate(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase) {
    const int blk = blockIdx.x;
    int lo = 0, hi = B - 1;                        // the largest b with tilebase[b] <= blk: at most 16 halvings
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tilebase[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    MmTile t;
    t.b = lo;
    t.d = desc + (size_t)lo * MM_DESC;
    t.H = t.d[1];
    t.W = t.d[2];
    const int k = blk - tilebase[lo], tw = (t.W + MM_TW - 1) / MM_TW;
    t.y0 = (k / tw) * MM_TH;
    t.x0 = (k % tw) * MM_TW;
    t.base = (size_t)pixbase[lo];
    return t;
}
// where an image's set lies after n active phases (one byte per pixel, != 0 is set), and where phase n + 1 writes
__device__ __forceinline__ const uint8_t* mm_src(const MmTile& t, int n, const uint8_t* buf, const uint8_t* pa, const uint8_t* pb) {
    return n == 0 ? buf + (size_t)t.d[0] : ((n & 1) ? pa : pb) + t.base;
}
__device__ __forceinline__ uint8_t* mm_dst(const MmTile& t, int n, uint8_t* pa, uint8_t* pb) { return (((n + 1) & 1) ? pa : pb) + t.base; }

// ---------------------------------------------------------------- scan
__global__ __launch_bounds__(MM_SCAN) void mm_scan_kernel(int B, const int32_t* __restrict__ desc, int32_t* __restrict__ pixbase, int32_t* __restrict__ tilebase,
                                                          int32_t* __restrict__ stats) {
    __shared__ int sp[MM_SCAN], st[MM_SCAN];
    const int tid = threadIdx.x, chunk = (B + MM_SCAN - 1) / MM_SCAN;
    const int b0 = min(tid * chunk, B), b1 = min(b0 + chunk, B);
    int p = 0, t = 0;
    for (int b = b0; b < b1; ++b) {
        const int H = desc[(size_t)b * MM_DESC + 1], W = desc[(size_t)b * MM_DESC + 2];
        p += H * W;                                // the host checked: the batch's pixels are below 2^31
        t += mm_tiles(H, W);
    }
    sp[tid] = p;
    st[tid] = t;
    __syncthreads();
    for (int o = 1; o < MM_SCAN; o <<= 1) {        // inclusive scan over the threads' sums
        const int ap = tid >= o ? sp[tid - o] : 0, at = tid >= o ? st[tid - o] : 0;
        __syncthreads();
        sp[tid] += ap;
        st[tid] += at;
        __syncthreads();
    }
    p = sp[tid] - p;                               // exclusive
    t = st[tid] - t;
    for (int b = b0; b < b1; ++b) {
        const int H = desc[(size_t)b * MM_DESC + 1], W = desc[(size_t)b * MM_DESC + 2];
        pixbase[b] = p;
        tilebase[b] = t;
        p += H * W;
        t += mm_tiles(H, W);
        int32_t* s = stats + (size_t)b * MM_DESC;
        s[0] = 0;
        s[1] = s[2] = INT_MAX;
        s[3] = s[4] = -1;
        s[5] = s[6] = s[7] = 0;
    }
    if (tid == MM_SCAN - 1) {
        pixbase[B] = sp[tid];
        tilebase[B] = st[tid];
    }
}

// ---------------------------------------------------------------- dilation-type pass
// LDS: (32 + 2r) rows of (64 + 2r) bytes, r the workgroup's own radius; the launch reserves it for the batch's largest radius of this phase.
__global__ __launch_bounds__(MM_THREADS) void mm_pass_kernel(int B, int phase, const uint8_t* __restrict__ buf, const int32_t* __restrict__ desc,
                                                             const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase, uint8_t* pa, uint8_t* pb) {
    extern __shared__ uint8_t g[];
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    const int r = (phase == MM_DILATE_C || phase == MM_ERODE_C) ? t.d[4] : t.d[5];
    if (r <= 0) return;                            // (uniform over the workgroup)
    const bool erode = phase == MM_ERODE_C || phase == MM_ERODE_O;
    const int n = mm_before(t.d, phase);
    const uint8_t* src = mm_src(t, n, buf, pa, pb);
    uint8_t* dst = mm_dst(t, n, pa, pb);
    const int tid = threadIdx.x, RW = MM_TW + 2 * r, RH = MM_TH + 2 * r, cap = r + 1;
    // 1. set / not set; a halo pixel outside the image is "not set" for both kinds
    for (int i = tid; i < RH * RW; i += MM_THREADS) {
        const int ry = i / RW, rx = i - ry * RW, y = t.y0 - r + ry, x = t.x0 - r + rx;
        bool set = false;
        if (y >= 0 && y < t.H && x >= 0 && x < t.W) set = (src[(size_t)y * t.W + x] != 0) != erode;
        g[i] = set ? 1 : 0;
    }
    __syncthreads();
    // 2. per column, in place: set -> the distance to the nearest set pixel of the column, capped at r + 1 (a set pixel: 0)
    if (tid < RW) {
        int d = cap;
        for (int ry = 0; ry < RH; ++ry) {
            d = g[ry * RW + tid] ? 0 : min(d + 1, cap);
            g[ry * RW + tid] = (uint8_t)d;
        }
        d = cap;
        for (int ry = RH - 1; ry >= 0; --ry) {
            d = min((int)g[ry * RW + tid], min(d + 1, cap));
            g[ry * RW + tid] = (uint8_t)d;
        }
    }
    __syncthreads();
    // 3. per pixel: within r of the set?
    const int rr = r * r;
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, ty = i / MM_TW, tx = i % MM_TW, y = t.y0 + ty, x = t.x0 + tx;
        if (y >= t.H || x >= t.W) continue;
        const uint8_t* row = g + (ty + r) * RW + tx + r;
        int c = row[0];
        bool hit = c <= r;                         // dx = 0: g <= r
        for (int dx = 1; dx <= r && !hit; ++dx) {
            const int a = row[-dx], b2 = row[dx];
            c = min(a, b2);
            hit = c * c + dx * dx <= rr;
        }
        dst[(size_t)y * t.W + x] = (hit != erode) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- hole fill: components.hip's union-find on the background
__device__ __forceinline__ int mm_find_lds(volatile int* lab, int x) {
    int n;
    while ((n = lab[x]) != x) x = n;               // strictly decreasing: lab[x] <= x
    return x;
}
__device__ __forceinline__ void mm_union_lds(int* lab, int a, int b) {
    for (;;) {
        a = mm_find_lds(lab, a);
        b = mm_find_lds(lab, b);
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

__global__ __launch_bounds__(MM_THREADS) void mm_tile_kernel(int B, const uint8_t* __restrict__ buf, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                             const int32_t* __restrict__ tilebase, const uint8_t* pa, const uint8_t* pb, int32_t* __restrict__ label,
                                                             int32_t* __restrict__ area) {
    __shared__ int lab[MM_TILE];
    __shared__ int cnt[MM_TILE];
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    if (t.d[6] == 0) return;                       // (uniform over the workgroup)
    const uint8_t* src = mm_src(t, mm_before(t.d, MM_FILL), buf, pa, pb);
    const int tid = threadIdx.x;
    const bool eight = t.d[7] == 8;
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        const bool bg = y < t.H && x < t.W && src[(size_t)y * t.W + x] == 0;
        lab[i] = bg ? i : -1;
        cnt[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, ty = i / MM_TW, tx = i % MM_TW;
        if (lab[i] < 0) continue;
        if (tx > 0 && lab[i - 1] >= 0) mm_union_lds(lab, i, i - 1);
        if (ty > 0) {
            if (lab[i - MM_TW] >= 0) mm_union_lds(lab, i, i - MM_TW);
            if (eight) {
                if (tx > 0 && lab[i - MM_TW - 1] >= 0) mm_union_lds(lab, i, i - MM_TW - 1);
                if (tx < MM_TW - 1 && lab[i - MM_TW + 1] >= 0) mm_union_lds(lab, i, i - MM_TW + 1);
            }
        }
    }
    __syncthreads();
    int root[MM_TILE / MM_THREADS];
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS;
        root[k] = lab[i] < 0 ? -1 : mm_find_lds(lab, i);      // (nothing is stored between the barriers: the forest stands still)
    }
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        if (root[k] < 0) continue;
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        atomicAdd(&cnt[root[k]], 1);               // at most 2048: the count never reaches the flag
        if (y == 0 || x == 0 || y == t.H - 1 || x == t.W - 1) atomicOr(&cnt[root[k]], MM_FRAME);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        if (y >= t.H || x >= t.W) continue;
        const size_t at = t.base + (size_t)y * t.W + x;
        const int r = root[k];
        label[at] = r < 0 ? -1 : (t.y0 + r / MM_TW) * t.W + t.x0 + r % MM_TW;
        area[at] = r == i ? cnt[i] : 0;
    }
}

__device__ __forceinline__ int mm_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int mm_find_global(const int32_t* lab, int x) {
    int n;
    while ((n = mm_load(lab + x)) != x) x = n;     // strictly decreasing whatever age the value read has
    return x;
}
__device__ __forceinline__ void mm_union_global(int32_t* lab, int a, int b) {
    for (;;) {
        a = mm_find_global(lab, a);
        b = mm_find_global(lab, b);
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

__global__ __launch_bounds__(MM_SEAM) void mm_seam_kernel(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase,
                                                          int32_t* __restrict__ label) {
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    if (t.d[6] == 0) return;
    const int tid = threadIdx.x;
    int y, x;
    if (tid < MM_TW) {
        y = t.y0;
        x = t.x0 + tid;
    } else if (tid < MM_TW + MM_TH) {
        y = t.y0 + tid - MM_TW;
        x = t.x0;
    } else {
        y = t.y0 + tid - MM_TW - MM_TH;
        x = t.x0 + MM_TW - 1;
    }
    if (y >= t.H || x >= t.W) return;
    int32_t* lab = label + t.base;
    const int W = t.W, p = y * W + x;
    if (mm_load(lab + p) < 0) return;
    const bool eight = t.d[7] == 8;
    // the neighbours of smaller raster index that lie in another tile: the pixel of the pair with the larger index does the union
    const bool top = y == t.y0 && y > 0, left = x == t.x0 && x > 0, right = x == t.x0 + MM_TW - 1 && x + 1 < W;
    if (left && mm_load(lab + p - 1) >= 0) mm_union_global(lab, p, p - 1);
    if (top && mm_load(lab + p - W) >= 0) mm_union_global(lab, p, p - W);
    if (eight && y > 0) {
        if (x > 0 && (top || left) && mm_load(lab + p - W - 1) >= 0) mm_union_global(lab, p, p - W - 1);
        if (x + 1 < W && (top || right) && mm_load(lab + p - W + 1) >= 0) mm_union_global(lab, p, p - W + 1);
    }
}

__global__ __launch_bounds__(MM_THREADS) void mm_flatten_kernel(int B, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase, const int32_t* __restrict__ tilebase,
                                                                int32_t* label, int32_t* area) {
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    if (t.d[6] == 0) return;
    volatile int32_t* lab = label + t.base;
    int32_t* ar = area + t.base;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        if (y >= t.H || x >= t.W) continue;
        const int p = y * t.W + x;
        int r = lab[p];
        if (r < 0) continue;
        int n;
        while ((n = lab[r]) != r) r = n;
        lab[p] = r;
        const int part = ar[p];                    // != 0 only at a tile-local root; only roots of whole components are added to, and they skip this
        if (part != 0 && r != p) {
            atomicAdd(&ar[r], part & MM_AREA);     // a component has fewer than 2^29 pixels: the sum never reaches the flag
            if (part & MM_FRAME) atomicOr(&ar[r], MM_FRAME);
        }
    }
}

__global__ __launch_bounds__(MM_THREADS) void mm_fill_kernel(int B, const uint8_t* __restrict__ buf, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                             const int32_t* __restrict__ tilebase, uint8_t* pa, uint8_t* pb, const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ area) {
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    const int hole_area = t.d[6];
    if (hole_area == 0) return;
    const int n = mm_before(t.d, MM_FILL);
    const uint8_t* src = mm_src(t, n, buf, pa, pb);
    uint8_t* dst = mm_dst(t, n, pa, pb);
    const int32_t* lab = label + t.base;
    const int32_t* ar = area + t.base;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        if (y >= t.H || x >= t.W) continue;
        const size_t p = (size_t)y * t.W + x;
        bool set = src[p] != 0;
        if (!set) {
            const int a = ar[lab[p]];              // a background pixel's label is its component's root after the flatten pass
            set = !(a & MM_FRAME) && (hole_area < 0 || (a & MM_AREA) <= hole_area);
        }
        dst[p] = set ? 1 : 0;
    }
}

// ---------------------------------------------------------------- final pass
__global__ __launch_bounds__(MM_THREADS) void mm_final_kernel(int B, uint8_t* buf, const int32_t* __restrict__ desc, const int32_t* __restrict__ pixbase,
                                                              const int32_t* __restrict__ tilebase, const uint8_t* pa, const uint8_t* pb, int32_t* __restrict__ stats) {
    __shared__ int st[8];
    const MmTile t = mm_locate(B, desc, pixbase, tilebase);
    uint8_t* m = buf + (size_t)t.d[0];
    uint8_t* ov = t.d[3] >= 0 ? buf + (size_t)t.d[3] : nullptr;
    const int n = mm_before(t.d, MM_FINAL);
    const uint8_t* res = n == 0 ? nullptr : ((n & 1) ? pa : pb) + t.base;      // no active phase: the mask is its own result
    const int tid = threadIdx.x;
    if (tid < 8) st[tid] = (tid == 1 || tid == 2) ? INT_MAX : ((tid == 3 || tid == 4) ? -1 : 0);
    __syncthreads();
    int after = 0, before = 0, added = 0, removed = 0, ymin = INT_MAX, xmin = INT_MAX, ymax = -1, xmax = -1;
#pragma unroll
    for (int k = 0; k < MM_TILE / MM_THREADS; ++k) {
        const int i = tid + k * MM_THREADS, y = t.y0 + i / MM_TW, x = t.x0 + i % MM_TW;
        if (y >= t.H || x >= t.W) continue;
        const size_t p = (size_t)y * t.W + x;
        const bool was = m[p] != 0, is = res ? res[p] != 0 : was;
        before += was;
        if (is) {
            ++after;
            ymin = min(ymin, y);
            ymax = max(ymax, y);
            xmin = min(xmin, x);
            xmax = max(xmax, x);
            if (!was) {
                ++added;
                m[p] = 255;
                if (ov) ov[3 * p + 1] = 255;
            }
        } else if (was) {
            ++removed;
            m[p] = 0;
            if (ov) ov[3 * p + 1] = ov[3 * p];
        }
    }
    if (after) {
        atomicAdd(&st[0], after);
        atomicMin(&st[1], ymin);
        atomicMin(&st[2], xmin);
        atomicMax(&st[3], ymax);
        atomicMax(&st[4], xmax);
    }
    if (added) atomicAdd(&st[5], added);
    if (removed) atomicAdd(&st[6], removed);
    if (before) atomicAdd(&st[7], before);
    __syncthreads();
    if (tid < 8) {
        int32_t* s = stats + (size_t)t.b * MM_DESC;
        const int v = st[tid];
        if (tid == 1 || tid == 2) {
            if (v != INT_MAX) atomicMin(&s[tid], v);
        } else if (tid == 3 || tid == 4) {
            if (v >= 0) atomicMax(&s[tid], v);
        } else if (v) {
            atomicAdd(&s[tid], v);
        }
    }
}

struct Range {
    uintptr_t lo, hi;
    int image;
    bool overlay;
};

}  // namespace

size_t uia_mask_morphology_ws_bytes(int B, int64_t pixels) {
    if (B < 1 || B > MM_MAX_B || pixels < 1 || pixels > 0x7fffffffLL) return 0;
    return mm_carve(nullptr, B, pixels).bytes;
}

int uia_mask_morphology_launch(hipStream_t stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats) {
    const char* who = "uia_mask_morphology";
    UIA_CHECK_ARG(B >= 1 && B <= MM_MAX_B, "%s: bad shape B=%d (1 <= B <= %d)", who, B, MM_MAX_B);
    UIA_CHECK_ARG(buf && desc && ws && stats, "%s: null tensor (buf, desc, ws and stats are required)", who);
    UIA_CHECK_ARG(buf_bytes >= 1 && buf_bytes <= 0x7fffffffu, "%s: a buffer of %zu bytes (1 .. 2^31 - 1: offsets are int32)", who, buf_bytes);
    UIA_CHECK_ARG((uintptr_t)ws % 8 == 0 && (uintptr_t)stats % 4 == 0, "%s: the workspace must be 8-byte, stats 4-byte aligned", who);
    std::vector<Range> ranges;
    ranges.reserve(2 * (size_t)B);
    unsigned long long pixels = 0, tiles = 0;
    int rc_max = 0, ro_max = 0;
    bool fill = false;
    for (int b = 0; b < B; ++b) {                                  // every image is checked before anything is enqueued
        const int32_t* d = desc + (size_t)b * MM_DESC;
        const long long moff = d[0], H = d[1], W = d[2], ooff = d[3], rc = d[4], ro = d[5], hole = d[6], conn = d[7];
        UIA_CHECK_ARG(H >= 1 && W >= 1 && H <= MM_MAX_SIDE && W <= MM_MAX_SIDE, "%s: image %d is %lld x %lld (1 .. %d a side)", who, b, H, W, MM_MAX_SIDE);
        UIA_CHECK_ARG(rc >= 0 && rc <= MM_MAX_R && ro >= 0 && ro <= MM_MAX_R, "%s: image %d has r_close %lld and r_open %lld (0 .. %d)", who, b, rc, ro, MM_MAX_R);
        UIA_CHECK_ARG(hole >= -1, "%s: image %d has hole_area %lld (-1: any size, 0: no fill, or the largest area filled)", who, b, hole);
        UIA_CHECK_ARG(conn == 4 || conn == 8, "%s: image %d has hole_connectivity %lld (4 or 8)", who, b, conn);
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
        tiles += (unsigned long long)mm_tiles((int)H, (int)W);
        rc_max = std::max(rc_max, (int)rc);
        ro_max = std::max(ro_max, (int)ro);
        fill = fill || hole != 0;
    }
    std::sort(ranges.begin(), ranges.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.image < b.image; });
    for (size_t i = 1; i < ranges.size(); ++i)                     // sorted by start: two ranges overlap iff some neighbours do
        UIA_CHECK_ARG(ranges[i - 1].hi <= ranges[i].lo, "%s: the %s of image %d overlaps the %s of image %d", who, ranges[i - 1].overlay ? "overlay" : "mask",
                      ranges[i - 1].image, ranges[i].overlay ? "overlay" : "mask", ranges[i].image);
    // the masks are disjoint parts of a buffer below 2^31 bytes, so the batch's pixels are below 2^31 as well
    const size_t need = uia_mask_morphology_ws_bytes(B, (int64_t)pixels);
    UIA_CHECK_ARG(need != 0 && ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    struct Fixed {
        uintptr_t lo, hi;
        const char* name;
    };
    const Fixed fixed[2] = {{(uintptr_t)stats, (uintptr_t)stats + (size_t)B * MM_DESC * sizeof(int32_t), "stats"}, {(uintptr_t)ws, (uintptr_t)ws + need, "the workspace"}};
    UIA_CHECK_ARG(!(fixed[0].lo < fixed[1].hi && fixed[1].lo < fixed[0].hi), "%s: %s overlaps %s", who, fixed[0].name, fixed[1].name);
    for (const Range& r : ranges)
        for (int i = 0; i < 2; ++i)
            UIA_CHECK_ARG(!(r.lo < fixed[i].hi && fixed[i].lo < r.hi), "%s: the %s of image %d overlaps %s", who, r.overlay ? "overlay" : "mask", r.image, fixed[i].name);

    const MmWs w = mm_carve(ws, B, (int64_t)pixels);
    const dim3 grid((unsigned)tiles), block(MM_THREADS);
    auto lds = [](int r) { return (size_t)(MM_TH + 2 * r) * (MM_TW + 2 * r); };
    UIA_CHECK_HIP(hipMemcpyAsync(w.desc, desc, (size_t)B * MM_DESC * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    mm_scan_kernel<<<dim3(1), dim3(MM_SCAN), 0, stream>>>(B, w.desc, w.pixbase, w.tilebase, stats);
    UIA_CHECK_LAUNCH();
    if (rc_max > 0) {
        mm_pass_kernel<<<grid, block, lds(rc_max), stream>>>(B, MM_DILATE_C, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1]);
        UIA_CHECK_LAUNCH();
        mm_pass_kernel<<<grid, block, lds(rc_max), stream>>>(B, MM_ERODE_C, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1]);
        UIA_CHECK_LAUNCH();
    }
    if (fill) {
        mm_tile_kernel<<<grid, block, 0, stream>>>(B, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1], w.label, w.area);
        UIA_CHECK_LAUNCH();
        if (tiles > (unsigned long long)B) {                       // some image has more than one tile
            mm_seam_kernel<<<grid, dim3(MM_SEAM), 0, stream>>>(B, w.desc, w.pixbase, w.tilebase, w.label);
            UIA_CHECK_LAUNCH();
        }
        mm_flatten_kernel<<<grid, block, 0, stream>>>(B, w.desc, w.pixbase, w.tilebase, w.label, w.area);
        UIA_CHECK_LAUNCH();
        mm_fill_kernel<<<grid, block, 0, stream>>>(B, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1], w.label, w.area);
        UIA_CHECK_LAUNCH();
    }
    if (ro_max > 0) {
        mm_pass_kernel<<<grid, block, lds(ro_max), stream>>>(B, MM_ERODE_O, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1]);
        UIA_CHECK_LAUNCH();
        mm_pass_kernel<<<grid, block, lds(ro_max), stream>>>(B, MM_DILATE_O, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1]);
        UIA_CHECK_LAUNCH();
    }
    mm_final_kernel<<<grid, block, 0, stream>>>(B, buf, w.desc, w.pixbase, w.tilebase, w.plane[0], w.plane[1], stats);
    UIA_CHECK_LAUNCH();
    return 0;
}
