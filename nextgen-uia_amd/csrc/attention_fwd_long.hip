// attention_fwd_long.hip — softmax(q kᵀ·scale) v for sequences of any length (head dim 64, no mask): online softmax over
// 64-key blocks, so no score row and no whole K / V of a head is ever held at once.
//
// Replaces: the plain-softmax MemEffAttention of the DINOv2 tower (the reference's src/third_party/dino/vision_transformer.py,
//           1370 tokens at 518 px) and every ViT of the library past the single-pass kernel's 272 tokens (attention_fwd.hip).
//
// Layout: that of attention_fwd.hip — element (b, l, h, d) of q / k / v is ptr[(b*L + l)*ld_qkv + h*64 + d] (read in place from the fused
// qkv rows), the output is row-major with its own leading dimension, lse (optional) is fp32 [B, H, L].
//
// bf16 path (MFMA 16x16x32, wave64): one workgroup per (batch, head, 128-query block), four waves of 32 queries (two 16-query tiles).
//   Q fragments stay in registers for the whole key sweep.  K and V arrive in 64-key blocks, double-buffered through LDS by register
//   staging: the global loads of block n+1 are issued before block n's products and written to the other buffer after them, one barrier
//   per block.  Scores are computed swapped (Sᵀ = K·Qᵀ, as in attention_fwd.hip) so that each lane owns one query: the block max and the
//   row sum are in-lane plus two lane swaps.  The running max m and sum l of a query are rescaled by exp2((m_old − m_new)·scale) when a
//   block raises the max (the factor is exactly 1 otherwise), and so is O; the exponentiated tile is, without lane movement, the B operand
//   of Oᵀ = Vᵀ·Pᵀ, with the Vᵀ fragments read from the row-major V tile by ds_read_b64_tr_b16.
// fp32 path (parity mode): one query per thread, 256 queries per workgroup; 64-key K / V blocks staged in LDS, online softmax over
//   16-key chunks on the VALU.
//
// Keys at or past L: the last block is partial; its K / V rows at or past L are never read (zeros are staged in their place) and their
// scores are −inf.  Reduction order is fixed (keys in ascending blocks, the lane-sum order of rows_sum): results are bit-identical from
// run to run.  Stores are per-lane vector stores.
#include "uia_common.h"
#include "uia_kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) char lds_char;
__device__ __forceinline__ s16x4 lds_tr16(const lds_char* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p); }

constexpr int KB = 64;                    // keys per block
constexpr int TILE_BYTES = KB * 128;      // one tensor's block in LDS: 64 rows of 64 bf16

// LONG_QT: 16-query tiles per wave; LONG_NW: waves per workgroup.  2 x 4: 32 KiB of LDS and 165 VGPRs per workgroup, three workgroups per CU.
constexpr int LONG_QT = 2, LONG_NW = 4;
constexpr int LONG_QBLK = 16 * LONG_QT * LONG_NW;

template <int QT, int NW>
__global__ __launch_bounds__(64 * NW, 2) void attn_fwd_long_bf16_kernel(const UiaAttnParams p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE_BYTES];   // [buffer][K | V][64 rows][128 B]
    constexpr int NSTG = KB * 8 / (64 * NW);                                 // 16-byte chunks per thread per tensor and block
    const int L = p.L;
    const int nqb = (L + 16 * QT * NW - 1) / (16 * QT * NW);
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb;
    const int b = bh / p.H, h = bh - b * p.H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)b * L;
    const size_t rs = (size_t)p.ld_qkv * 2;                                  // row stride in bytes
    const char* qb = (const char*)p.q + (row0 * p.ld_qkv + (size_t)h * 64) * 2;
    const char* kb = (const char*)p.k + (row0 * p.ld_qkv + (size_t)h * 64) * 2;
    const char* vb = (const char*)p.v + (row0 * p.ld_qkv + (size_t)h * 64) * 2;

    const int li = lane & 15, g = lane >> 4;
    const int q0row = 16 * QT * (NW * qblk + wave);                          // this wave's first query
    // ---- Q fragments (B operand, column = query li, k-slots = d 8g..8g+7 and 32+8g..): rows past L are clamped to L-1 (read, never stored)
    uint4 qa[QT], qc[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        int qr = q0row + 16 * j + li;
        qr = qr < L ? qr : L - 1;
        qa[j] = *(const uint4*)(qb + qr * rs + g * 16);
        qc[j] = *(const uint4*)(qb + qr * rs + (g + 4) * 16);
    }

    // ---- register staging of one 64-key block: chunk i = tid + 64·NW·n is row i>>3, 16-byte column chunk i&7.  K rows are stored with the
    //      chunk swizzle (row>>1)&7, V rows with ((row>>1)&3)<<1 (the transpose reads of attention_fwd.hip); rows at or past L are zeros.
    uint4 rk[NSTG], rv[NSTG];
    auto fetch = [&](int blk) {
#pragma unroll
        for (int n = 0; n < NSTG; ++n) {
            const int i = tid + 64 * NW * n, r = i >> 3, c = i & 7;
            const int gr = KB * blk + r;
            if (gr < L) {
                rk[n] = *(const uint4*)(kb + gr * rs + c * 16);
                rv[n] = *(const uint4*)(vb + gr * rs + c * 16);
            } else {
                rk[n] = uint4{0u, 0u, 0u, 0u};
                rv[n] = uint4{0u, 0u, 0u, 0u};
            }
        }
    };
    auto deposit = [&](int buf) {
        char* Ks = smem + buf * 2 * TILE_BYTES;
        char* Vs = Ks + TILE_BYTES;
#pragma unroll
        for (int n = 0; n < NSTG; ++n) {
            const int i = tid + 64 * NW * n, r = i >> 3, c = i & 7;
            *(uint4*)(Ks + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = rk[n];
            *(uint4*)(Vs + r * 128 + ((c ^ (((r >> 1) & 3) << 1)) << 4)) = rv[n];
        }
    };

    const float sc = p.scale * 1.44269504088896341f;                         // softmax in base 2
    // K fragment (A operand, rows = keys): row 16t+li, chunks g and g+4 under the swizzle (li>>1)
    const int offK0 = li * 128 + ((g ^ (li >> 1)) << 4);
    // Vᵀ fragment by transpose read: rows 32u + 16hh + 4g + (li>>2), columns 16dt + 4(li&3)
    const int vrow0 = 4 * g + (li >> 2), vsw = (vrow0 >> 1) & 3;
    int voff[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) voff[dt] = TILE_BYTES + vrow0 * 128 + ((dt ^ vsw) << 5) + 8 * (li & 3);

    f32x4 o[QT][4];
    float m[QT], l[QT];                                                      // running max of the RAW scores (scale > 0), lane-partial running sum
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        m[j] = -INFINITY;
        l[j] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int nkb = (L + KB - 1) / KB;
    fetch(0);
    deposit(0);
    __syncthreads();
    for (int blk = 0; blk < nkb; ++blk) {
        const bool more = blk + 1 < nkb;
        if (more) fetch(blk + 1);                                            // in flight under this block's products
        const int buf = blk & 1;
        const char* Ks = smem + buf * 2 * TILE_BYTES;
        const lds_char* Ls = (const lds_char*)(smem + buf * 2 * TILE_BYTES);

        // ---- Sᵀ = K·Qᵀ: s[j][t][r] = score of query (tile j, column li) against key 64·blk + 16t + 4g + r
        f32x4 s[QT][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint4 k0 = *(const uint4*)(Ks + t * 2048 + offK0);
            const uint4 k1 = *(const uint4*)(Ks + t * 2048 + (offK0 ^ 64));
#pragma unroll
            for (int j = 0; j < QT; ++j) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k0), __builtin_bit_cast(bf16x8, qa[j]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, k1), __builtin_bit_cast(bf16x8, qc[j]), acc, 0, 0, 0);
                s[j][t] = acc;
            }
        }
        const int nvalid = L - KB * blk;                                     // wave-uniform; >= 1
        if (nvalid < KB) {
#pragma unroll
            for (int j = 0; j < QT; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[j][t][r] = (16 * t + 4 * g + r) < nvalid ? s[j][t][r] : -INFINITY;
        }
        // ---- online softmax: new max, rescale of l and O, exponentials
#pragma unroll
        for (int j = 0; j < QT; ++j) {
            float mb = s[j][0][0];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) mb = fmaxf(mb, s[j][t][r]);
            mb = rows_max(mb);                                               // finite: every block holds a valid key
            const float mn = fmaxf(m[j], mb);
            const float alpha = __builtin_amdgcn_exp2f((m[j] - mn) * sc);   // 0 on the first block (m = −inf), 1 when the max did not grow
            m[j] = mn;
            const float msc = mn * sc;
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __builtin_amdgcn_exp2f(fmaf(s[j][t][r], sc, -msc));   // exp2(−inf) = 0 for keys past L
                    s[j][t][r] = e;
                    sum += e;
                }
            l[j] = fmaf(l[j], alpha, sum);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[j][dt][r] *= alpha;
        }
        // ---- Oᵀ += Vᵀ·Pᵀ over the two 32-key halves (k-slot (g,e) of half u ↔ key 32u + 16(e>>2) + 4g + (e&3))
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            bf16x8 pf[QT];
#pragma unroll
            for (int j = 0; j < QT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    pf[j][e] = (bf16_t)s[j][2 * u][e];
                    pf[j][4 + e] = (bf16_t)s[j][2 * u + 1][e];
                }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const lds_char* base = Ls + voff[dt] + 32 * 128 * u;
                const s16x4 lo = lds_tr16(base);
                const s16x4 hi = lds_tr16(base + 16 * 128);
                const s16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int j = 0; j < QT; ++j)
                    o[j][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf), pf[j], o[j][dt], 0, 0, 0);
            }
        }
        if (more) deposit(buf ^ 1);                                          // the other buffer: every wave left it at the previous barrier
        __syncthreads();
    }

    // ---- store: lane owns query q0row + 16j + li, d = 16dt + 4g + r
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const float tot = rows_sum(l[j]);
        const int qrow = q0row + 16 * j + li;
        if (qrow < L) {
            const float inv = 1.0f / tot;
            bf16_t* orow = (bf16_t*)p.out + (row0 + qrow) * p.ldo + (size_t)h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) store4(orow + 16 * dt, f32x4{o[j][dt][0] * inv, o[j][dt][1] * inv, o[j][dt][2] * inv, o[j][dt][3] * inv});
            if (p.lse && g == 0) p.lse[((size_t)b * p.H + h) * L + qrow] = (m[j] * sc + log2f(tot)) * 0.69314718055994531f;
        }
    }
}

// ------------------------------------------------------------------------------------------
// fp32 parity path: one query per thread; K / V blocks of 64 keys broadcast from LDS; online softmax over 16-key chunks.
constexpr int F32_Q = 256, F32_CH = 16;

__global__ __launch_bounds__(F32_Q) void attn_fwd_long_f32_kernel(const UiaAttnParams p) {
    __shared__ __attribute__((aligned(16))) float Ks[KB * 64];
    __shared__ __attribute__((aligned(16))) float Vs[KB * 64];
    const int L = p.L;
    const int nqb = (L + F32_Q - 1) / F32_Q;
    const int bh = blockIdx.x / nqb, qblk = blockIdx.x - bh * nqb;
    const int b = bh / p.H, h = bh - b * p.H;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)b * L;
    const float* qb = (const float*)p.q + row0 * p.ld_qkv + (size_t)h * 64;
    const float* kb = (const float*)p.k + row0 * p.ld_qkv + (size_t)h * 64;
    const float* vb = (const float*)p.v + row0 * p.ld_qkv + (size_t)h * 64;
    const int qi = F32_Q * qblk + tid;
    const int qr = qi < L ? qi : L - 1;                                     // rows past L: a valid row is read, nothing is stored
    float q[64];
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const f32x4 v = *(const f32x4*)(qb + (size_t)qr * p.ld_qkv + c);
        q[c] = v[0] * p.scale; q[c + 1] = v[1] * p.scale; q[c + 2] = v[2] * p.scale; q[c + 3] = v[3] * p.scale;
    }
    float o[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) o[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int nkb = (L + KB - 1) / KB;
    for (int blk = 0; blk < nkb; ++blk) {
        __syncthreads();                                                     // every thread is done with the previous block
        for (int i = tid; i < KB * 16; i += F32_Q) {
            const int r = i >> 4, c = (i & 15) * 4, gr = KB * blk + r;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *(f32x4*)(Ks + r * 64 + c) = gr < L ? *(const f32x4*)(kb + (size_t)gr * p.ld_qkv + c) : z;
            *(f32x4*)(Vs + r * 64 + c) = gr < L ? *(const f32x4*)(vb + (size_t)gr * p.ld_qkv + c) : z;
        }
        __syncthreads();
        const int nvalid = L - KB * blk < KB ? L - KB * blk : KB;
        for (int k0 = 0; k0 < nvalid; k0 += F32_CH) {
            float s[F32_CH];
            float cm = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < F32_CH; ++kk) {
                float a = 0.f;
#pragma unroll
                for (int c = 0; c < 64; ++c) a = fmaf(q[c], Ks[(k0 + kk) * 64 + c], a);
                s[kk] = k0 + kk < nvalid ? a : -INFINITY;
                cm = fmaxf(cm, s[kk]);
            }
            const float mn = fmaxf(m, cm);
            const float alpha = expf(m - mn);                                // 0 on the first chunk, 1 when the max did not grow
            m = mn;
            l *= alpha;
#pragma unroll
            for (int c = 0; c < 64; ++c) o[c] *= alpha;
#pragma unroll
            for (int kk = 0; kk < F32_CH; ++kk) {
                const float e = expf(s[kk] - mn);
                l += e;
#pragma unroll
                for (int c = 0; c < 64; ++c) o[c] = fmaf(e, Vs[(k0 + kk) * 64 + c], o[c]);
            }
        }
    }
    if (qi < L) {
        const float inv = 1.0f / l;
        float* orow = (float*)p.out + (row0 + qi) * p.ldo + (size_t)h * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 4) *(f32x4*)(orow + c) = f32x4{o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv};
        if (p.lse) p.lse[((size_t)b * p.H + h) * L + qi] = m + logf(l);
    }
}

}  // namespace

int uia_attn_fwd_long_launch(hipStream_t stream, int dtype, const UiaAttnParams& p) {
    UIA_CHECK_ARG(dtype == UIA_BF16 || dtype == UIA_F32, "uia_attn_fwd_long: bad dtype %d", dtype);
    UIA_CHECK_ARG(p.B > 0 && p.H > 0 && p.L > 0, "uia_attn_fwd_long: empty problem");
    UIA_CHECK_ARG(p.dh == 64, "uia_attn_fwd_long: head dim %d, only 64 is supported", p.dh);
    UIA_CHECK_ARG(p.mask_kind == UIA_MASK_NONE, "uia_attn_fwd_long: no mask is supported (mask kind %d)", p.mask_kind);
    UIA_CHECK_ARG(!p.cu_seqlens, "uia_attn_fwd_long: packed sequences (cu_seqlens) are not supported");
    UIA_CHECK_ARG(p.out_kb_rows == 0 && p.dqkv_kb_rows == 0, "uia_attn_fwd_long: the output must be row-major (no K-blocked output)");
    UIA_CHECK_ARG(p.scale > 0.f && p.scale < 3.0e38f, "uia_attn_fwd_long: scale must be positive and finite (the row max is taken on the raw scores), got %g", (double)p.scale);
    UIA_CHECK_ARG(p.q && p.k && p.v && p.out, "uia_attn_fwd_long: null tensor");
    const int esz = dtype == UIA_BF16 ? 2 : 4;
    UIA_CHECK_ARG(p.ld_qkv >= 64 * p.H && p.ldo >= 64 * p.H, "uia_attn_fwd_long: leading dimensions (%lld, %lld) narrower than H*64 = %d",
                  (long long)p.ld_qkv, (long long)p.ldo, 64 * p.H);
    UIA_CHECK_ARG((p.ld_qkv * esz) % 16 == 0 && (p.ldo * esz) % 16 == 0, "uia_attn_fwd_long: leading dimensions must keep 16-byte rows");
    UIA_CHECK_ARG(((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.out) % 16 == 0, "uia_attn_fwd_long: pointers must be 16-byte aligned");
    UIA_CHECK_ARG(!p.lse || (uintptr_t)p.lse % 4 == 0, "uia_attn_fwd_long: lse alignment");
    const long long heads = (long long)p.B * p.H;
    if (dtype == UIA_F32) {
        const long long grid = heads * ((p.L + F32_Q - 1) / F32_Q);
        UIA_CHECK_ARG(grid < (1ll << 31), "uia_attn_fwd_long: grid too large");
        hipLaunchKernelGGL(attn_fwd_long_f32_kernel, dim3((unsigned)grid), dim3(F32_Q), 0, stream, p);
        UIA_CHECK_LAUNCH();
        return 0;
    }
    const long long grid = heads * ((p.L + LONG_QBLK - 1) / LONG_QBLK);
    UIA_CHECK_ARG(grid < (1ll << 31), "uia_attn_fwd_long: grid too large");
    hipLaunchKernelGGL((attn_fwd_long_bf16_kernel<LONG_QT, LONG_NW>), dim3((unsigned)grid), dim3(64 * LONG_NW), 0, stream, p);
    UIA_CHECK_LAUNCH();
    return 0;
}
