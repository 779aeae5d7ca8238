/* uia_hip.h — C ABI of libuia_hip.so: the MI355X (gfx950) kernels behind the CLIP-adapter
 * fine-tune hot path of jinggqu/NextGen-UIA.
 *
 * The reference is pure Python on stock PyTorch and has NO native boundary of its own; what a
 * maintainer would bind is the set of ATen calls its hot path makes.  Each entry point below names
 * the reference call sites (file:line under /root/reference) whose arithmetic it replaces.
 * INTEGRATION.md shows the ctypes binding and the module-level swap-in.
 *
 * Contract (every function):
 *   - extern "C", returns 0 on success, <0 on error; uia_last_error() gives a thread-local message.
 *   - no allocation inside: the caller owns every buffer (PyTorch device tensors → data_ptr()).
 *   - asynchronous on the hipStream_t passed as `stream` (torch.cuda.current_stream().cuda_stream);
 *     no internal threads, no host synchronisation, graph-capturable.
 *   - one process per GPU; the only global state is the RCCL communicator of uia_comm_*.
 *   - dtype: UIA_F32 (parity mode, exact-fp32 MFMA / VALU) or UIA_BF16 (operands bf16, fp32
 *     accumulate).  "T" below means that element type.  The residual stream, losses, parameter
 *     gradients and optimiser state are fp32 in both modes.
 *   - tensors are row-major and contiguous unless a leading dimension (in elements) is given;
 *     16-byte alignment of every base pointer and row is required and checked.
 */
#ifndef UIA_HIP_H
#define UIA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { UIA_F32 = 0, UIA_BF16 = 1 };
enum { UIA_ACT_NONE = 0, UIA_ACT_GELU = 1, UIA_ACT_QUICKGELU = 2, UIA_ACT_RELU = 3 };
enum { UIA_MASK_NONE = 0, UIA_MASK_CAUSAL = 1, UIA_MASK_KEYPAD = 2 };
enum { UIA_MONA_BASELINE = 0, UIA_MONA_NOISE_AWARE = 1, UIA_MONA_FREQ_ENHANCED = 2, UIA_MONA_HYBRID = 3 };

const char* uia_last_error(void);
int uia_version(void);

/* ---------------------------------------------------------------------------------------------
 * Dense contraction  C[M,N] = epilogue(alpha · A[M,K] · W[N,K]ᵀ)   (both operands K-contiguous).
 * Replaces every nn.Linear / F.linear / addmm of the path:
 *   src/third_party/openai_clip/model.py:181-188,197,200-201,255,372  (in_proj, out_proj, c_fc, c_proj, proj)
 *   src/adapters/mona.py:127,148 (project1 / project2)      src/adapters/lora.py:80,87 (base + rank factors)
 *   timm Attention.qkv/proj, Mlp.fc1/fc2; HF BertSelfAttention / BertIntermediate / BertOutput  [third-party]
 * and, run against the cached transpose Wᵀ, their autograd dgrad  dx = dy·W.
 * Epilogue order: v = alpha·acc + bias;  aux_out ← v;  v = act(v);  v *= act'(aux_in)  (dact);
 *                 v += resid (fp32);  v += residT (T);  out32 ← v;  outT ← v.
 * Requirements: K % (128/sizeof(T)) == 0, N % 8 == 0. */
typedef struct uia_gemm_desc {
    const void* A; int64_t lda;
    const void* W; int64_t ldw;
    int32_t M, N, K;
    float alpha;
    const float* bias;
    int32_t act;
    int32_t dact;
    const void* aux_in; int64_t ldaux_in;
    void* aux_out; int64_t ldaux_out;
    const float* resid; int64_t ldr;
    int32_t resid_mod, resid_row_off;   /* resid_mod>0: residual row = m % resid_mod + resid_row_off (pos-embed) */
    const void* residT; int64_t ldrT;
    int32_t out_group;                  /* >0: output row = m + m/out_group + 1 (patch rows -> token rows, CLS slot skipped) */
    void* outT; int64_t ldo;
    float* out32; int64_t ldo32;
    int32_t w_kblocked;                 /* 1: W is stored K-blocked, [K/g][N][g] with g = 64 bytes / sizeof(T) elements (ldw ignored): the layout
                                           the ring tile configs (8, 10; the automatic choice for M > 2048, N > 64) stream fastest; other tile
                                           configs reject it */
    const void* resid_ln_stats;         /* non-null: `resid` holds the INPUT of a LayerNorm and the residual added is that LayerNorm's output,
                                           fmaf((resid[m][n] - mean_m)·rstd_m, resid_ln_w[n], resid_ln_b[n]) with (mean_m, rstd_m) =
                                           resid_ln_stats[2m], [2m+1] as written by uia_layernorm_fwd_stats: a post-LN (BERT) sub-layer sum
                                           then reads the previous sum once instead of the LayerNorm writing its fp32 output for it
                                           (HF BertSelfOutput / BertOutput: LayerNorm(dense(h) + input_tensor) [third-party]) */
    const float* resid_ln_w;
    const float* resid_ln_b;
    /* LayerNorm folded into the GEMMs on either side of it (frozen affine; timm Block norm1 / norm2 and HF BertSelfOutput / BertOutput
     * LayerNorm [third-party], model.py:163-169 + 181-202 for the OpenAI blocks): the PRODUCER of the normalised rows x adds their row
     * sums to `rowsum_out` while it stores them (and can write their T copy through outT beside out32); the CONSUMER takes that T copy of
     * the RAW rows as A and a weight whose columns are pre-scaled by the LayerNorm weight, W'[n][k] = W[n][k]·ln_w[k], and evaluates
     *     LN(x)·Wᵀ + b  =  rstd_m·(x·W'ᵀ − mean_m·colsum[n]) + (b + W·ln_b)[n]
     * in its epilogue (the caller passes colsum[n] = Σ_k W'[n][k] and the combined bias as `bias`), so the stand-alone LayerNorm pass
     * over the rows (read 4 B, write 2 B per element) disappears. */
    int64_t* rowsum_out;                /* non-null: rowsum_out[2m] += Σ_n v[m][n], rowsum_out[2m+1] += Σ_n v[m][n]² over the N columns of the fp32
                                           result v this launch stores, as 64-bit FIXED-POINT numbers in units of 2^-30 (integer atomics: the
                                           sums do not depend on the order in which a row's column tiles arrive; caller zeroes; 16-byte aligned) */
    const int64_t* lnfold_sums;         /* non-null: A holds raw rows; (Σ, Σ²) of row m over lnfold_dim columns at lnfold_sums[2m], [2m+1],
                                           in the fixed-point form rowsum_out leaves them */
    const float* lnfold_colsum;         /* [N] fp32 column sums of the pre-scaled weight */
    int32_t lnfold_dim; float lnfold_eps;
    int32_t resid_ln_dim; float resid_ln_eps;   /* resid_ln_dim > 0: resid_ln_stats points at (Σ, Σ²) over resid_ln_dim columns as rowsum_out leaves
                                                   them (int64 fixed point), not at float (mean, rstd); mean = Σ/dim, rstd = rsqrt(max(Σ²/dim − mean², 0) + resid_ln_eps) */
    /* K-BLOCKED ACTIVATIONS (ring tile configs with 64-byte sub-tiles: 8, 10, 13, 14; the other configs reject them).  The operand of a
     * large GEMM streams fastest as [K·sizeof(T)/64][rows][64 bytes] (each 1 KiB LDS-DMA piece = 8 whole 128-byte lines; +1.5…3.4 % per
     * launch on the step's shapes, profiles/r02_a_gemm_order_layout.txt).  A GEMM whose T result is the next GEMM's A operand can write it
     * in that layout directly, and the consumer reads it with a_kb_rows set:
     *   a_kb_rows    > 0: A is K-blocked; element (m, k) is at A[((k / g)·a_kb_rows + m)·g + k % g], g = 64 / sizeof(T) (lda ignored).
     *                     a_kb_rows is the row count of the WHOLE K-blocked tensor (its plane stride), A may point at a row offset in it.
     *   outT_kb_rows > 0: the T output is written K-blocked the same way, column n playing the part of k (N·sizeof(T) % 64 == 0; ldo ignored). */
    int64_t a_kb_rows;
    int64_t outT_kb_rows;
    /* Guard of the folded LayerNorms (optional; a caller-owned, caller-zeroed device word that many launches may share).  The fold hands
     * the GEMM bf16(x) instead of bf16(LN(x)): fine for roughly centred rows, lossy for |mean| >> std.  Every launch that carries
     * rowsum_out / lnfold_sums / resid_ln_dim checks the rows it touches and ORs into *ln_flag
     *   bit 0: a consumer saw a row with |mean|·rstd > ln_flag_limit   (the caller should go back to the stand-alone LayerNorm kernels)
     *   bit 1: a producer's partial row sum was non-finite or outside the fixed-point range (|Σ| or Σ² >= 5e8 per wave column; the partial
     *          is clamped so that the integer atomics cannot wrap, and the statistics of that row are garbage: the caller must fail loudly)
     * The atomics are issued only for offending rows, so a healthy step pays one compare per row. */
    int32_t* ln_flag;
    float ln_flag_limit;                /* <= 0: 8.0 */
    /* LoRA input dropout (/root/reference/src/adapters/lora.py:82-83) without a pass of its own.  keep(seed, element index) is the generator
     * of uia_dropout (eight consecutive elements per draw), so a fused launch and uia_dropout + a plain launch see the same mask.
     *   drop_where = 1: the A operand is dropped while it streams through the N = 64 kernel (tile cfg 16; element (m, k) has index m·K + k);
     *                   a_drop_out, if set, receives the dropped rows ([M, K], leading dimension lda) for the weight gradient.
     *   drop_where = 2: alpha·acc (+ bias, activation) of output element (m, n), index m·N + n, is dropped before the residual adds:
     *                   dx += drop(s·q·A), the backward of the same dropout (run-time epilogue; N % 8 == 0). */
    int32_t drop_where;
    float drop_p;
    uint64_t drop_seed;
    void* a_drop_out;
    /* SPLIT K for launches of a few tiles and a long K (the M tail of a large GEMM: its cost is the latency of the K chain, not work).  Two calls with
     * the SAME descriptor on tile config 13 (half-height tiles, run-time epilogue): 13 | slices << 16 | 1 << 22 runs one workgroup per (tile, K slice),
     * each adding its raw fp32 accumulators into the tile's image in splitk_ws (hardware float atomics); 13 | slices << 16 | 2 << 22 reads the image,
     * zeroes it again and runs the epilogue.  splitk_ws: tiles · 128·256 floats (tiles = ceil(M/128)·ceil(N/256)), 16-byte aligned, caller-owned,
     * ZERO before the first use (the launches keep it zero between uses).  The slice partials meet in no fixed order: last-bit run-to-run variation. */
    float* splitk_ws;
    /* K EXTENSION: the LoRA rank update inside the frozen GEMM (y = x·Wᵀ + s·t·Bᵀ as ONE K loop over [x | t]·[W | s·B]ᵀ; lora.py:87).  K counts BOTH parts
     * and W holds K columns; A supplies the first K − K2 of them (row-major, lda), A2 the last K2: a row-major [M, K2] operand (lda2) per group of
     * a2_group_cols output columns, group g at A2 + g·a2_group_stride elements (a fused q | k | v projection has three; 0 = one operand for all columns).
     * bf16, tile cfgs 8 / 13, K2 % 32 == 0, a2_group_cols % 256 == 0. */
    const void* A2;
    int64_t lda2;
    int32_t K2;
    int32_t a2_group_cols;
    int64_t a2_group_stride;
    /* THREE-BYTE fp32 tensors for the HBM-bound epilogues of a frozen post-LN tower (bf16 launches): a value x is kept as hi = bf16(x) (round to
     * nearest: the T copy the next GEMM reads as its A operand anyway) plus lo = the next 8 mantissa bits as a signed byte,
     *     float_bits(x) ≈ (hi_bits << 16) + (lo << 8)      (15 stored mantissa bits: 2^-16 relative),
     * so a sub-layer sum costs 3 + 3 bytes per element in the epilogue that reads one and writes the next, instead of 4 + (4 + 2).
     * lo = ((bits + 0x80) >> 8) - (hi_bits << 8) lies in [-128, 128] and is clamped to +-127: the decoded value is within 2^-16 of x (relative)
     * where the clamp did not act, within 2^-15 where it did (1 value in 256), within 256 * 2^-149 (absolute) for subnormal x.
     * INPUT CONDITION: |x| below the float with bits 0x7F7F8000 (3.39618e38).  From there on the round-to-nearest hi plane is inf (the T copy a
     * GEMM reads), and from bits 0x7F7FFF80 on the decoded value is inf too, although x is finite.  (tests/layernorm_reference.py proves the figures.)
     *   resid_lo8 != NULL: the residual is (residT, resid_lo8) in that form — residT row-major (ldrT) or, residT_kb_rows > 0, K-blocked like
     *                      outT; `resid` must be NULL; resid_ln_* (stats / weight / bias / dim) then apply to the reconstructed rows.
     *   out_lo8   != NULL: the result's low bytes go there (row-major, ld_out_lo), its hi plane is outT (required); out32 may be NULL.
     *   resid_lo_kb_rows / out_lo_kb_rows > 0: that plane of low bytes is column-blocked like the K-blocked hi plane, 64 columns (64 bytes) per
     *                      block with that many rows: byte (m, n) at ((n / 64)·rows + m)·64 + n % 64 — a 16-row pass of the epilogue then
     *                      moves whole 128-byte lines instead of 64-byte pieces 768 bytes apart (N % 64 == 0). */
    const int8_t* resid_lo8;
    int64_t ld_resid_lo;
    int64_t residT_kb_rows;
    int8_t* out_lo8;
    int64_t ld_out_lo;
    int64_t resid_lo_kb_rows;
    int64_t out_lo_kb_rows;
} uia_gemm_desc;
/* tile_cfg: 0 = chosen from the shape (what every caller in this repo passes unless it runs an experiment).  Low byte = a kernel: 8 the 256 x 256 ring tile (eight
 * waves, LDS-DMA), 13 / 14 its half-height forms, 12 persistent, 16 / 23 the N = 64 / K = 64 streams, 24 five-deep ring, 25 / 26 four waves of 128 x 128, 27 / 28 / 29 the same
 * with operands staged through registers (two / three sub-tiles in flight / a persistent grid; bf16, no K extension, operands below 4 GiB), 1-5 / 21 small tiles; bits 8-15 =
 * row panels per tile-order group (255 = none).  Every ring kernel returns bit-identical results for a given descriptor; an unsupported combination returns -1. */
int uia_gemm(void* stream, int dtype, const uia_gemm_desc* d, int tile_cfg /* 0 = auto */);

/* Parameter gradient of a Linear:  dW[I,J] += Σ_m A[m,I]ᵀ·B[m,J]  and optionally dbias[I] += Σ_m A[m,I]
 * (fp32 accumulate with atomics into caller-zeroed buffers).  One of I, J must be ≤ 64·k.
 * Replaces autograd's wgrad of mona.py:127,148 and lora.py:87. */
int uia_wgrad(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb,
              float alpha, float* dW, float* dbias_A);
/* The same with the operands zero-padded to the kernel's 64-wide tiles and the gradient not: only rows < i_valid and columns < j_valid are
 * accumulated, into dW with leading dimension ldw — a LoRA factor's [out, r] / [r, in] gradient (r = 16 padded to 64) lands in the
 * parameter's own .grad without a padded staging buffer, its zero fill and its slice copy (lora.py:87). */
int uia_wgrad_ex(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb,
                 float alpha, float* dW, int64_t ldw, int i_valid, int j_valid, float* dbias_A);
/* dW[I,J] += alpha * A.T @ drop(B): the LoRA factor gradient dA = s * q.T @ dropout(x) (lora.py:82-87) with the dropout REGENERATED while B is staged —
 * B holds the un-dropped rows, a window of J columns starting at column drop_col0 of a [M, drop_ld] tensor whose mask uia_dropout /
 * uia_gemm_desc.drop_where = 1 draw from (seed, element index / 8); the forward then need not write the dropped rows out.  bf16; extents as uia_wgrad_ex. */
int uia_wgrad_drop(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb,
                   float alpha, float* dW, int64_t ldw, int i_valid, int j_valid, float drop_p, uint64_t seed, int64_t drop_ld, int drop_col0);
/* Up to four weight gradients of ONE shape in one launch (the q | k | v factors of a LoRA attention block, lora.py:82-87 three times: three launches of short-lived workgroups
 * were three latencies).  Problem g: dW[g][i_valid, j_valid] += alpha * A[g].T @ drop_g(B[g]) (+ dbias_A[g] += column sums of A[g] where given, without dropout only); all problems
 * share M, I, J, the leading dimensions, alpha, the valid extent and the dropout window; drop_p = 0: no dropout, else problem g's mask is drawn from drop_seed[g] as uia_wgrad_drop
 * draws it.  bf16.  Same arithmetic per problem as uia_wgrad_ex / uia_wgrad_drop. */
typedef struct uia_wgrad_group_desc {
    int32_t n, M, I, J;
    const void* A[4];
    const void* B[4];
    float* dW[4];
    float* dbias_A[4];
    int64_t lda, ldb, ldw;
    int32_t i_valid, j_valid;
    float alpha, drop_p;
    uint64_t drop_seed[4];
    int64_t drop_ld;
    int32_t drop_col0, reserved;
} uia_wgrad_group_desc;
int uia_wgrad_group(void* stream, int dtype, const uia_wgrad_group_desc* d);

/* ---------------------------------------------------------------------------------------------
 * softmax(q kᵀ·scale + mask) v, head dim 64, L <= 272, one workgroup per (batch, head).
 * Replaces nn.MultiheadAttention (model.py:195-197), F.scaled_dot_product_attention
 * (src/adapters/lora.py:188; timm Attention [third-party]), HF BertSelfAttention [third-party].
 * Element (b,l,h,d) of q/k/v is ptr[(b*L+l)*ld_qkv + h*64 + d]; likewise out/dout/dq/dk/dv. */
typedef struct uia_attn_desc {
    const void *q, *k, *v; int64_t ld_qkv;
    void* out; int64_t ldo;
    float* lse;               /* [B,H,L] fp32 log-sum-exp of the scaled scores (fwd: written if non-null) */
    const int32_t* keylen;    /* [B] valid keys (UIA_MASK_KEYPAD) */
    int32_t B, H, L, dh;
    int32_t mask_kind;
    float scale;
    const void* dout; int64_t lddo;              /* backward only */
    void *dq, *dk, *dv; int64_t ld_dqkv;         /* backward only */
    const int32_t* cu_seqlens; /* forward only, optional: [B+1] row offsets of PACKED (un-padded) sequences; sequence b then has
                                  cu[b+1]-cu[b] <= L tokens at rows cu[b].. and every key is valid (L is the maximum length) */
    /* bf16, dh = 64: K-blocked tensors on the GEMM side of the attention (uia_gemm_desc.a_kb_rows; g = 32 elements).
     *   out_kb_rows  > 0: `out` is K-blocked with that many rows — written so by the forward (it is the A operand of the output
     *                     projection), read so by the backward; element (row, h, d) is at out[((2h + d/32)·out_kb_rows + row)·32 + d%32].
     *   dqkv_kb_rows > 0: backward: dq, dk, dv are written K-blocked the same way (dq / dk / dv each point at the first column block
     *                     of their part of the fused [rows, 3·H·64] gradient, the A operand of the QKV data-gradient GEMM). */
    int64_t out_kb_rows;
    int64_t dqkv_kb_rows;
} uia_attn_desc;
int uia_attn_fwd(void* stream, int dtype, const uia_attn_desc* d);
int uia_attn_bwd(void* stream, int dtype, const uia_attn_desc* d);
/* Same backward with an explicit kernel configuration (bf16, dh = 64; ignored otherwise): 0 = the library's choice (what uia_attn_bwd
 * runs), 1 = the lock-step 8-wave kernel (dS crosses LDS once per 32-query block), 2 / 3 / 4 = the barrier-free unit kernel (waves pull
 * key-tile and query-tile units from an LDS counter; no product of one wave is read by another) with 8 waves and V in LDS / 4 waves and
 * V fragments from global memory (two heads per CU up to 208 tokens) / 8 waves and V from global memory (2 stages the O rows that δ needs
 * through LDS up to 240 tokens; 6 = 2 with those operands from global memory at every length); 5 = the persistent form of
 * the unit kernel (one workgroup per CU walks the heads, the next head's operands land under the current head's sweeps; L <= 240).
 * For A/B timing and tests. */
int uia_attn_bwd_cfg(void* stream, int dtype, const uia_attn_desc* d, int cfg);

/* softmax(q kᵀ·scale) v for sequences of any length L >= 1 (uia_attn_fwd stops at 272): online softmax over 64-key blocks, one
 * workgroup per (batch, head, query block).  Head dim 64, no mask, no cu_seqlens, row-major out (out_kb_rows = 0); lse is written if
 * non-null.  q / k / v / out 16-byte aligned, ld_qkv and ldo rows of whole 16-byte units.  Forward only (no long backward).
 * Replaces the MemEffAttention of the DINOv2 tower (third_party/dino/vision_transformer.py [third-party], 1370 tokens at 518 px). */
int uia_attn_fwd_long(void* stream, int dtype, const uia_attn_desc* d);

/* uia_attn_bwd for a dout that is zero outside token 0 of every sequence (the CLS pool of a contrastive head): `dout` holds the B non-zero rows
 * only, row b at dout[b·lddo + h·64 + d], and q, out and lse are read at token 0.  With P_j = exp(scale·q_0·k_j − lse_0) and δ = dout·out_0:
 * dv_j = P_j·dout, dk_j = P_j(dout·v_j − δ)·scale·q_0, dq_0 = Σ_j P_j(dout·v_j − δ)·scale·k_j and dq_l = 0 for l > 0.  EVERY element of dq, dk and dv
 * is written (the zero rows too), row-major or K-blocked (dqkv_kb_rows) as uia_attn_bwd writes them; out row-major or K-blocked (out_kb_rows).
 * bf16 and fp32, head dim 64, L <= 288, mask kind none only; every pointer 16-byte aligned, every leading dimension a whole number of 16-byte units. */
int uia_attn_bwd_cls(void* stream, int dtype, const uia_attn_desc* d);

/* The forward twin, for a caller that reads token 0 of the attention output and nothing else: the ONE query row q_0 of every (sequence, head) against
 * the keys j < n, n = L (mask kind none, keylen null) or max(min(keylen[b], L), 1) (UIA_MASK_KEYPAD: the clamp uia_attn_fwd applies to an all-padding
 * sequence).  s_j = scale·q_0·k_j, m = max_j s_j, P_j = exp(s_j − m), l = Σ_j P_j; out[b·ldo + h·64 + d] = Σ_j P_j v_j[d] / l — B compact rows, not
 * B·L — and lse[b·H + h] = m + log l when lse is non-null.  q / k / v are addressed as in uia_attn_fwd (element (b,l,h,d) at ptr[(b·L+l)·ld_qkv + h·64 + d]);
 * no K or V row at or beyond n is read.  The sums over the keys run in a fixed order: two launches on the same operands give the same bits.
 * bf16 and fp32, head dim 64, L <= 288, row-major out (out_kb_rows = 0), no cu_seqlens; q / k / v / out 16-byte aligned, ld_qkv and ldo whole 16-byte units. */
int uia_attn_fwd_cls(void* stream, int dtype, const uia_attn_desc* d);
/* uia_attn_bwd_cls on what uia_attn_fwd_cls left: `out` is [B, H·64] (row b at out[b·ldo + h·64 + d], row-major) and `lse` is [B, H]; everything else
 * — q / k / v, dout, the dense dq / dk / dv, row-major or K-blocked — as uia_attn_bwd_cls. */
int uia_attn_bwd_cls_rows(void* stream, int dtype, const uia_attn_desc* d);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over fp32 rows (model.py:163-169; timm / HF LayerNorm [third-party]).
 * x rows may be strided by ldx (elements); y / dy are compact [M,D].  Backward is for FROZEN
 * gamma/beta (dx only): dx = dres + LN'(dy); statistics are recomputed from x. */
int uia_layernorm_fwd(void* stream, int dtype, int M, int D, int64_t ldx, const float* x, const float* gamma, const float* beta,
                      float eps, void* yT, float* y32);
/* Same, and additionally stats[2m] = mean_m, stats[2m+1] = rstd_m (fp32) when `stats` is non-null; yT and y32 may then both be null
 * only if stats is given.  The deferred-residual form of uia_gemm (resid_ln_stats) consumes them. */
int uia_layernorm_fwd_stats(void* stream, int dtype, int M, int D, int64_t ldx, const float* x, const float* gamma, const float* beta,
                            float eps, void* yT, float* y32, float* stats);
/* out[b, :] = mean over rows l in [row0, row0+n) of LayerNorm(x[b, l, :]) (fp32; token rows ldx elements apart, images L·ldx apart;
 * out rows ldo apart).  The patch-token pool of the DINOv2 classification head (dino/dinov2.py:33-100 [third-party]) without a
 * normalised [B·L, D] tensor.  ws: B·UIA_POOL_SLICES·D floats of scratch.  Fixed summation order (bit-identical runs).
 * D <= 1024, D % 4 == 0, every pointer 16-byte aligned. */
#define UIA_POOL_SLICES 32
int uia_ln_mean_rows(void* stream, int B, int L, int row0, int n, int D, int64_t ldx, const float* x, const float* gamma, const float* beta,
                     float eps, float* ws, float* out, int64_t ldo);
int uia_layernorm_bwd(void* stream, int dtype, int M, int D, int64_t ldx, const void* dy, const float* x, const float* gamma,
                      float eps, const float* dres, float* dx32, void* dxT);
/* The same backward on THREE-BYTE tensors (bf16 launches, compact rows; the form is defined at uia_gemm_desc.resid_lo8): inside a frozen block
 * the attention-half output x1 and its gradient dx1 never exist in fp32 — x1 leaves the output projection's epilogue as (T copy, low bytes) and
 * is read here for the statistics; dx1 leaves this kernel as (dxT, dx_lo) and comes back as the next call's (dres_hi, dres_lo).
 *   x_lo   != NULL: x is (x_hi, x_lo); x must be NULL; x_hi row-major [M, D] or, x_kb_rows > 0, K-blocked with that many rows per 32-column block.
 *   dres_lo != NULL: dres is (dres_hi, dres_lo); dres must be NULL; dres_hi row-major or, dres_kb_rows > 0, K-blocked like x_hi (the T copy a row kernel
 *                    left for a ring GEMM is also the hi plane of the residual gradient).      dx_lo != NULL: the result is (dxT, dx_lo); dx32 may be NULL. */
int uia_layernorm_bwd3(void* stream, int dtype, int M, int D, int64_t ldx, const void* dy, const float* x, const void* x_hi, const int8_t* x_lo, int64_t x_kb_rows,
                       const float* gamma, float eps, const float* dres, const void* dres_hi, const int8_t* dres_lo, int64_t dres_kb_rows, float* dx32, void* dxT,
                       int8_t* dx_lo);
/* The same backward with a PERIODIC residual gradient: rows r with r % period == 0 take dres_rows[r / period] (compact fp32 [ceil(M / period), D]), every
 * other row has none — the gradient of a block's residual stream when only token 0 of every `period` tokens carries one.  Bit-identical to
 * uia_layernorm_bwd3 on dres_rows zero-padded to [M, D].  Compact rows (ldx == D).  Forms: bf16 with a three-byte result (dx_lo != NULL; x fp32 or
 * three-byte as above) and fp32 (dx32 and / or dxT, x fp32). */
int uia_layernorm_bwd_periodic(void* stream, int dtype, int M, int D, const void* dy, const float* x, const void* x_hi, const int8_t* x_lo, int64_t x_kb_rows,
                               const float* gamma, float eps, const float* dres_rows, int period, float* dx32, void* dxT, int8_t* dx_lo);

/* ---------------------------------------------------------------------------------------------
 * Mona adapter, all four variants (src/adapters/mona.py:75-487; equations SURVEY.md Appendix E.1).
 * The two projections run on uia_gemm, their weight gradients on uia_wgrad; these are the stages
 * in between.  bottleneck must be 64.
 *   pre_fwd      u = LN(x; norm.w, norm.b, eps)*gamma + x*gammax                  (mona.py:125,227,328,461)
 *   spatial_fwd  t [B,1+h*w,64] -> d = dropout(gelu([t_cls ; op(t_spatial)]))      (mona.py:129-147 + *MonaOp.forward)
 *   spatial_bwd  dd -> dt and += gradients of every adapter_conv parameter (fp32 atomics, caller zeroes)
 *   pre_bwd      dx = dy + du*gammax + LN'(du*gamma*norm.w); += d gamma, gammax, norm.w, norm.b
 * Dropout: keep_mask (uint8 [B,1+h*w,64]) if non-null, else the counter hash of (seed, element index)
 * when p_drop > 0; kept values are scaled by 1/(1-p_drop).  Pass the same seed / mask to fwd and bwd. */
typedef struct uia_mona_spatial_desc {
    int32_t variant, B, h, w, bott;
    const void* t;                /* T [B, 1+h*w, bott] output of project1 */
    void* d;                      /* T [B, 1+h*w, bott] forward output (input of project2) */
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *conv3_w, *conv3_b;   /* depth-wise 3x3 / 5x5 / 7x7 */
    const float *proj_w, *proj_b;                                             /* 1x1 projector [64,64] */
    const float* freq;                                                        /* freq_filter [64] (freq_enhanced, hybrid) */
    const float *ne1_w, *ne1_b, *ne3_w, *ne3_b;                               /* noise_estimator.{1,3} (noise_aware, hybrid) */
    float p_drop; uint64_t seed; const uint8_t* keep_mask;
    const void* dd;               /* backward: T grad wrt d */
    void* dt;                     /* backward: T grad wrt t */
    float *g_conv1_w, *g_conv1_b, *g_conv2_w, *g_conv2_b, *g_conv3_w, *g_conv3_b, *g_proj_w, *g_proj_b, *g_freq,
          *g_ne1_w, *g_ne1_b, *g_ne3_w, *g_ne3_b;
    float* ws;                    /* backward, optional: uia_mona_spatial_workspace_bytes(B) of scratch. With it every image writes one
                                     partial-gradient row and a second kernel adds the column sums into g_* in a fixed order
                                     (deterministic, no atomic contention); without it the kernel uses float atomics. */
} uia_mona_spatial_desc;
size_t uia_mona_spatial_workspace_bytes(int B);
int uia_mona_pre_fwd(void* stream, int dtype, int M, int D, const float* x, const float* norm_w, const float* norm_b,
                     const float* gamma, const float* gammax, float eps, void* u);
/* uia_mona_pre_fwd with project1 inside (bf16, D = 768, bottleneck 64): also writes t = u @ w1.T + b1 (mona.py:126-127), w1 = project1.weight [64, D] row-major,
 * t [M, ldt >= 64]; bit-identical to uia_mona_pre_fwd followed by uia_gemm on the N = 64 stream kernel. */
int uia_mona_pre_fwd_t(void* stream, int dtype, int M, int D, const float* x, const float* norm_w, const float* norm_b, const float* gamma, const float* gammax,
                       float eps, void* u, const void* w1, int64_t ldw1, const float* b1, void* t, int64_t ldt);
int uia_mona_pre_bwd(void* stream, int dtype, int M, int D, const void* du, const float* x, const float* dy,
                     const float* norm_w, const float* norm_b, const float* gamma, const float* gammax, float eps,
                     float* dx32, void* dxT, float* g_gamma, float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws,
                     int64_t dxT_kb_rows);
/* dxT_kb_rows > 0: the T copy of dx is written K-blocked, [D/g][dxT_kb_rows][g] with g = 64 / sizeof(T) elements (uia_gemm_desc.a_kb_rows):
 * it is the A operand of the preceding block's fc2 data-gradient GEMM and of nothing else.
 * ws: caller-owned scratch of uia_mona_pre_bwd_workspace_bytes(M, D) bytes (per-workgroup partial rows of the four parameter
 * gradients, summed by a second small launch: a direct atomic add from every workgroup serialises on the same 4*D addresses) */
/* The same with project1's data gradient inside (bf16, bottleneck 64, D % 64 == 0, D <= 768): du = dt @ W1 is computed per 16-row tile on the matrix cores
 * from dt [M, 64] (the gradient wrt project1's output, mona.py:127) and w1t = project1.weight transposed, [D, 64] row-major, instead of being read
 * from a [M, D] tensor a K = 64 GEMM launch wrote; identical results (same products, same bf16 rounding of du). */
int uia_mona_pre_bwd_du(void* stream, int dtype, int M, int D, const void* dt, int64_t ldt, const void* w1t, int64_t ldw1, const float* x, const float* dy,
                        const float* norm_w, const float* norm_b, const float* gamma, const float* gammax, float eps,
                        float* dx32, void* dxT, float* g_gamma, float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws, int64_t dxT_kb_rows);
/* uia_mona_pre_bwd_du on THREE-BYTE residual gradients (the form of uia_gemm_desc.resid_lo8; reference: the fp32 gradient autograd hands mona.py:151's residual add):
 * dy arrives as (dy_hi bf16 row-major [M, D], dy_lo int8 [M, D]) — what uia_layernorm_bwd3 left as (dxT, dx_lo) — and dx leaves as (dxT, dx_lo), dxT row-major or,
 * dxT_kb_rows > 0, K-blocked: 3 bytes read and 3 written per element of the stream instead of 4 and 4 + 2.  Same arithmetic as uia_mona_pre_bwd_du on the decoded values. */
int uia_mona_pre_bwd_du3(void* stream, int dtype, int M, int D, const void* dt, int64_t ldt, const void* w1t, int64_t ldw1, const float* x, const void* dy_hi, const int8_t* dy_lo,
                         const float* norm_w, const float* norm_b, const float* gamma, const float* gammax, float eps, void* dxT, int8_t* dx_lo, float* g_gamma,
                         float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws, int64_t dxT_kb_rows);
size_t uia_mona_pre_bwd_workspace_bytes(int M, int D);
int uia_mona_spatial_fwd(void* stream, int dtype, const uia_mona_spatial_desc* d);
int uia_mona_spatial_bwd(void* stream, int dtype, const uia_mona_spatial_desc* d);
/* The CLS token's share of uia_mona_spatial_bwd alone (the token bypasses the spatial operator, mona.py:132,139), for a gradient that is zero on
 * every other token: dt[b, c] = dd[b, c] · keep(b·ntok·64 + c) · gelu'(t[b·ldt + c]) with compact dd / dt [B, 64] and t the CLS rows of project1's
 * output, ldt elements apart (ntok·64 on the saved tensor).  The dropout mask is indexed as in the dense tensor of ntok tokens per image, so the
 * regenerated mask (or keep_mask, uint8 [B, ntok, 64]) is the forward's; bit-identical to the CLS rows uia_mona_spatial_bwd writes.  The
 * adapter_conv parameters get no gradient from this token. */
int uia_mona_cls_bwd(void* stream, int dtype, int B, int ntok, const void* dd, const void* t, int64_t ldt, void* dt, float p_drop, uint64_t seed,
                     const uint8_t* keep_mask);
/* Its forward twin, the CLS token's share of uia_mona_spatial_fwd alone: d[b, c] = keep(b·ntok·64 + c) · gelu(t[b·ldt + c]) with compact d [B, 64] and t the
 * CLS rows of project1's output, ldt elements apart (64 on a compact [B, 64] tensor).  ntok is the token count of the DENSE tensor the mask is indexed in
 * (seed, or keep_mask uint8 [B, ntok, 64]): bit-identical to the CLS rows uia_mona_spatial_fwd writes for the same t, and uia_mona_cls_bwd with the
 * same (ntok, p_drop, seed / keep_mask) regenerates the same mask. */
int uia_mona_cls_fwd(void* stream, int dtype, int B, int ntok, const void* t, int64_t ldt, void* d, float p_drop, uint64_t seed, const uint8_t* keep_mask);

/* The WHOLE adapter forward of mona.py:319-362 (and :96-151, :198-253, :427-487) in one launch, one workgroup per image:
 *     y = x + project2(drop(gelu(spatial(project1(LN(x)·gamma + x·gammax)))))
 * pre -> project1 (768 -> 64 on MFMA, W1 resident in LDS) -> the spatial op on the fp32 [tokens][64] LDS tile -> GELU / dropout ->
 * project2 (64 -> 768 on MFMA, W2 fragments in registers) + residual, with u, t and d never travelling through HBM between stages.
 * bf16 only, bottleneck 64, grid width 14 or 4, D % 128 == 0, D <= 768 (uia_mona_fused_supported says whether a shape qualifies; everything
 * else runs as uia_mona_pre_fwd -> uia_gemm -> uia_mona_spatial_fwd -> uia_gemm with identical semantics).
 *   sp      variant, B, h, w, bott, the adapter_conv parameters, p_drop / seed / keep_mask;  sp.d (optional): T [B,1+hw,64] copy of d for the
 *           backward's weight gradient;  sp.t, sp.dd, sp.dt, sp.g_*, sp.ws are ignored
 *   x       fp32 [B,1+hw,D];  norm_w/norm_b/gamma/gammax fp32 [D];  w1 T [64,D] (project1.weight), b1 fp32 [64];  w2 T [D,64] (project2.weight), b2 fp32 [D]
 *   y32     fp32 [B,1+hw,D];  yT (optional) its T copy: row-major, or K-blocked with yT_kb_rows > 0 (uia_gemm_desc.a_kb_rows);
 *   rowsum_out (optional) receives (Σ, Σ²) of every row of y in the fixed-point form of uia_gemm_desc.rowsum_out — STORED, not added
 *           (an image's rows belong to one workgroup); ln_flag as in uia_gemm_desc
 *   u_out, t_out (optional) T [B·(1+hw), D] / [B,1+hw,64]: u and t for the backward (uia_wgrad of project1 / uia_mona_spatial_bwd) */
typedef struct uia_mona_fused_desc {
    uia_mona_spatial_desc sp;
    int32_t D; float eps;
    const float* x;
    const float *norm_w, *norm_b, *gamma, *gammax;
    const void* w1; const float* b1;
    const void* w2; const float* b2;
    float* y32;
    void* yT; int64_t yT_kb_rows;
    int64_t* rowsum_out;
    int32_t* ln_flag;
    void* u_out;
    void* t_out;
} uia_mona_fused_desc;
int uia_mona_fused_supported(int dtype, int D, int h, int w, int bott);
int uia_mona_fused_fwd(void* stream, int dtype, const uia_mona_fused_desc* d);

/* ---- LoRA rank update of a data gradient, up to three sources in one pass (csrc/lora_rank.hip) ----
 * Replaces, in the backward of the reference's LinearLoRA (src/adapters/lora.py:78-90: result += dropout(x) @ A.T @ B.T * scaling, one nn.Dropout per
 * wrapped Linear) applied to q, k and v of an OpenAI-CLIP block (inject_lora_to_clip, lora.py:115-199), the three read-modify-write launches
 *     dh += mask_i * (alpha * Q_i @ W_i.T) / (1 - p)        Q_i = dy_i @ B_i  [M, 64] (rank zero-padded to 64),  W_i = A_i.T  [N, 64]
 * by ONE pass over dh.  bf16; N % 256 == 0 and nsrc * N/4 * 144 bytes <= 160 KB (N <= 1024 with three sources).
 *   Q        bf16 [nsrc][M][ldq >= 64]; source s starts q_stride elements after source s-1
 *   W[s]     bf16 [N][ldw >= 64]
 *   out      bf16 [M][ldo >= N], read and written in place
 *   drop_p   0 = no dropout; otherwise mask_s is drawn per 8 output columns from (seed[s], (m*N + n) / 8) exactly as uia_dropout /
 *            uia_gemm_desc.drop_where = 2 draw it for an [M, N] tensor, so the forward's masks are reproduced from the seeds alone */
typedef struct uia_lora_rank_desc {
    int32_t M, N, nsrc;
    float alpha;
    const void* Q; int64_t ldq, q_stride;
    const void* W[3]; int64_t ldw;
    void* out; int64_t ldo;
    float drop_p;
    uint64_t seed[3];
} uia_lora_rank_desc;
int uia_lora_rank_update(void* stream, int dtype, const uia_lora_rank_desc* d);

/* LayerNorm + the down-projections of up to three LinearLoRA wrappers that share the input (q, k, v of an OpenAI-CLIP block; reference lora.py:82-87:
 * dropout(x) @ A.T, one nn.Dropout per wrapper) in one launch:  h = LayerNorm(x) (written, bf16 [M, D]) and  T[s] = dropout_s(h) @ A[s][:16].T.
 * bf16, D = 768 or 1024, rank <= 16 (A[s]: bf16 [>= 16, lda >= D], the first 16 rows are used); T: bf16 [nsrc][M][64] (t_stride elements between
 * sources), columns 0..15 hold the products and 16..63 zeros (the K-extension operand of uia_gemm_desc.A2 is 64 wide).  drop_p = 0: no dropout; otherwise
 * mask_s is the mask uia_gemm_desc.drop_where = 1 / uia_dropout draw for the [M, D] tensor h from seed[s] — uia_wgrad_drop regenerates it in the backward. */
typedef struct uia_ln_lora_desc {
    int32_t M, D, nsrc;
    float eps;
    const float* x; int64_t ldx;
    const float *gamma, *beta;
    void* h;
    const void* A[3]; int64_t lda;
    void* T; int64_t t_stride;
    float drop_p;
    uint64_t seed[3];
} uia_ln_lora_desc;
int uia_ln_lora_down(void* stream, int dtype, const uia_ln_lora_desc* d);

/* ---------------------------------------------------------------------------------------------
 * Task heads of the feature-pyramid adapter (reference src/third_party/timm/clip_adapter.py:47-57, 118-160).
 * uia_upsample_bilinear_fwd: nn.Upsample((H,W), mode="bilinear", align_corners=False) of a token-major map
 *   src[(b*h*w + y*w + x)*ld + c] -> dst[b][c][Y][X] (NCHW fp32).  _bwd: dsrc (token-major, overwritten) from ddst (NCHW),
 *   as a gather (fixed summation order).  The reference's Conv1x1 after the upsample is applied BEFORE it by the caller
 *   (it commutes with the interpolation), so C here is the number of classes.
 * uia_segment_mean_fwd: out[b][c] = mean_i x[(b*n + i)*ld + c]  (AdaptiveAvgPool2d(1) + Flatten); _bwd broadcasts dout/n. */
int uia_upsample_bilinear_fwd(void* stream, int B, int C, int h, int w, int H, int W, const float* src, int64_t ld, float* dst);
int uia_upsample_bilinear_bwd(void* stream, int B, int C, int h, int w, int H, int W, const float* ddst, float* dsrc, int64_t ld);
int uia_segment_mean_fwd(void* stream, int B, int n, int C, const float* x, int64_t ld, float* out);
int uia_segment_mean_bwd(void* stream, int B, int n, int C, const float* dout, float* dx, int64_t ld);
/* MONAI DiceCELoss(to_onehot_y=True, softmax=True, squared_pred=True, smooth_nr, smooth_dr) of the segmentation entry points
 * (reference src/models/clipseg/segmentation.py:84, biomedclip/segmentation.py:75): loss (one float) and d loss / d logits in
 * one call.  logits, dlogits fp32 [B,C,H*W] (NCHW), label fp32 [B,H*W] holding class indices, 2 <= C <= 8;
 * ws: uia_dicece_workspace_bytes(B) of scratch. */
size_t uia_dicece_workspace_bytes(int B);
int uia_dicece_fwd_bwd(void* stream, int B, int C, int HW, const float* logits, const float* label, float smooth_nr, float smooth_dr,
                       float* ws, float* loss, float* dlogits);
/* MONAI FocalLoss(to_onehot_y=True) in its sigmoid form, mean reduction, of the classification entry points (reference
 * src/models/biomedclip/classification.py:77): loss (one float, the mean over all N*C elements) and d loss / d logits in one call.
 * logits, dlogits fp32 [N,C]; labels int64 [N], target one_hot(label); 2 <= C <= 64, 1 <= N <= 2^20; gamma >= 0; alpha < 0 means none,
 * else the element weight is t*alpha + (1-t)*(1-alpha).  A label outside [0, C) makes the loss (and its row of dlogits) NaN; it is never an index.
 * Deterministic (fixed-order two-stage sum in fp64, no atomics).  ws: uia_focal_workspace_bytes(N, C) of scratch. */
size_t uia_focal_workspace_bytes(int N, int C);
int uia_focal_fwd_bwd(void* stream, int N, int C, const float* logits, const int64_t* labels, float gamma, float alpha, void* ws, size_t ws_bytes,
                      float* loss, float* dlogits);
/* Binary classification counts and AUROC of a split (torchmetrics Accuracy / Precision / Recall / F1Score / AUROC, task="binary").
 * p1 fp32 [N] (probability of class 1), labels int64 [N] in {0,1}, perm int64 [N]: the permutation that sorts p1 ascending; 1 <= N <= 2^24.
 * record fp64 [5]: TP, FP, TN, FN at p1 > 0.5 (strict) and the exact tie-aware AUROC (ties count 1/2 = the trapezoidal ROC area; 0.0 when a
 * class is absent).  A label outside {0,1} or a perm entry outside [0,N) makes every field NaN.  ws: uia_binary_cls_stats_workspace_bytes(N). */
size_t uia_binary_cls_stats_workspace_bytes(int N);
int uia_binary_cls_stats(void* stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes, double* record);
/* Surface-distance metrics of the segmentation MetricAccumulator (reference src/utils/tools.py:185-206: MONAI 1.5.1 compute_hausdorff_distance(
 * include_background=False, percentile=95) and compute_average_surface_distance(include_background=False, symmetric=False), spacing=None).
 * logits fp32 [B,2,H,W], label fp32 [B,1,H,W]; 1 <= H, W <= 1024, B >= 1.  Per image: P = argmax(logits) == 1 (tie -> class 0, NaN is the maximum),
 * G = label > 0, edges E(M) = M & ~erode(M) (4-neighbour, out of image = background), d(A->B) = float32 exact Euclidean pixel distance from each
 * pixel of E(A) to the nearest pixel of E(B).  hd[b] = max(q(d(P->G)), q(d(G->P))) with q = torch.quantile(d, percentile / 100) (0 <= percentile
 * <= 100; percentile 0 is the maximum, as in MONAI), asd[b] = mean of d(P->G); both fp64, NaN when P or G is empty.  Unit spacing in both axes: a
 * physical spacing would scale the two axes of the integer squared distance.  Deterministic (integer selection, fixed-order fp64 sums, no float
 * atomics).  ws: uia_surface_distances_workspace_bytes(B, H, W) of scratch (about 14 bytes per pixel). */
size_t uia_surface_distances_workspace_bytes(int B, int H, int W);
int uia_surface_distances(void* stream, int B, int H, int W, const float* logits, const float* label, float percentile, void* ws, size_t ws_bytes,
                          double* hd, double* asd);
/* The three pictures of the segmentation test pass (reference src/utils/tools.py:278-315, visualize_seg: `(images * 255).astype(np.uint8)`,
 * `torch.argmax(preds, dim=1)`, the np.maximum overlays, one image at a time on the host), for a whole batch in one launch.
 * logits fp32 [B,C,S,S] with C == 2, contiguous; images fp32 [B,Ci,S,S] with Ci 1 or 3, of which channel 0 is read; labels [B,1,S,S] as uint8
 * (label_dtype UIA_SEG_LABEL_U8) or fp32 (UIA_SEG_LABEL_F32); B >= 1, 1 <= S <= 16384, B*S*S <= 2^36; fp32 inputs on 4-byte addresses.
 * Per pixel: g = (uint8)(x * 255), the product rounded once to fp32, clamped to [0, 255] with NaN -> 0 (numpy leaves out-of-range values undefined), then
 * truncated; t = 255 where label != 0, else 0; p = 255 where argmax over the two logits is class 1 by torch's rules (a tie, -0.0 against +0.0 included,
 * goes to class 0; NaN is the maximum; NaN in both goes to class 0), the prediction uia_surface_distances and the Dice / IoU metrics use, else 0.
 * Outputs, caller-owned uint8, plain row-major with no PNG filter bytes: mask_rgb [B,S,S,3] = (t, p, 0), overlay_rgb [B,S,S,3] =
 * (max(g,t), max(g,p), g), pred [B,S,S] = p.  Every byte of the three is written, nothing beside them.
 * Everything is checked before anything is enqueued (non-zero, uia_last_error(), nothing written): null pointers, B or S out of range, C != 2,
 * Ci not 1 or 3, an unknown label_dtype, an output that overlaps another output or an input.  Asynchronous, deterministic, no workspace.
 * uia_seg_viz_form: 1 when the call runs on the four-pixels-per-thread kernel (16-byte loads, dword stores): S % 4 == 0, logits, images and fp32
 * labels on 16-byte addresses, uint8 labels and the three outputs on 4-byte addresses; 0 for the pixel-per-thread kernel with byte stores that takes
 * everything else.  A pure function of its arguments: no GPU is needed. */
enum { UIA_SEG_LABEL_U8 = 0, UIA_SEG_LABEL_F32 = 1 };
int uia_seg_viz_form(int S, int label_dtype, const void* logits, const void* images, const void* labels, const void* mask_rgb, const void* overlay_rgb,
                     const void* pred);
int uia_seg_viz(void* stream, int B, int C, int Ci, int S, const float* logits, const float* images, const void* labels, int label_dtype,
                uint8_t* mask_rgb, uint8_t* overlay_rgb, uint8_t* pred);
/* Image-text retrieval evaluation (the call sites of reference src/models/biomedclip/retrieval.py:329; the reference never shipped its metric module, so
 * these definitions are this build's).  img, txt fp32 [N,E] row-major contiguous, 16-byte aligned: N feature pairs; 1 <= N <= 2^24, E % 4 == 0,
 * 4 <= E <= 4096.  Scores s_ij = <a_i, b_j> with a_i = img_i / max(||img_i||, 1e-12), b_j likewise from txt_j (F.normalize) when normalize != 0, else
 * the raw rows; the product runs on the exact fp32 MFMA (a k-ordered fmaf chain from 0), and the bits of s_ij depend only on the values of row i of img
 * and row j of txt, never on their place in a tile or the grid: equal pairs of rows give exact ties.  d_i = s_ii comes from the same tile path.
 * Outputs int32 [N] each, for image i: gt_i2t[i] = #{j != i : s_ij > d_i}, eq_i2t[i] = #{j != i : s_ij == d_i}; for text j: gt_t2i[j] =
 * #{i != j : s_ij > d_j}, eq_t2i[j] = #{i != j : s_ij == d_j}.  IEEE comparisons (a NaN score is neither greater nor equal); a query whose own d is
 * not finite gets gt = N - 1, eq = 0 (the worst rank).  Ranks are OPTIMISTIC: rank = 1 + gt, the (sim > diag).sum() form; eq counts the others tied
 * with the query's own pair.  The N x N matrix is never written; rows, columns and k of the padding are masked by index.  The call zeroes its own
 * outputs (they may be uninitialised), is asynchronous and deterministic (integer atomics only).
 * ws: uia_retrieval_workspace_bytes(N, E) of scratch (the diagonal and the two normalised copies; 0 for a shape outside the limits). */
size_t uia_retrieval_workspace_bytes(int N, int E);
int uia_retrieval_ranks(void* stream, int N, int E, const float* img, const float* txt, int normalize, void* ws, size_t ws_bytes,
                        int32_t* gt_i2t, int32_t* eq_i2t, int32_t* gt_t2i, int32_t* eq_t2i);
/* Statistics of one retrieval direction.  gt int32 [N] on the device (uia_retrieval_ranks), k_values a HOST array of nk values, 1 <= nk <= 16, every
 * K >= 1 (checked before any launch); 1 <= N <= 2^24.  With rank = 1 + gt, record fp64 [nk + 2] on the device: record[t] = 100 * #{rank <= K_t} / N
 * (R@K), record[nk] the median rank (the two middle values averaged for even N, as numpy.median), record[nk + 1] the mean rank.  rsum is the sum of
 * every R@K of both directions (two records).  Integer counting and selection, an exact integer rank sum; no float atomics.
 * ws: uia_retrieval_stats_workspace_bytes(N) of scratch. */
size_t uia_retrieval_stats_workspace_bytes(int N);
int uia_retrieval_stats(void* stream, int N, const int32_t* gt, int nk, const int32_t* k_values, void* ws, size_t ws_bytes, double* record);
/* Top-K listing: each query's K best gallery rows, from the score tiles of uia_retrieval_ranks with a selection epilogue; the Q x N matrix is never
 * written.  queries fp32 [Q,E], gallery fp32 [N,E], row-major contiguous, 16-byte aligned; 1 <= Q, N <= 2^24, E % 4 == 0, 4 <= E <= 4096,
 * 1 <= K <= min(N, 32).  Scores s_qj = <a_q, b_j> with the rows divided by max(||row||, 1e-12) when normalize != 0: the same k-ordered fmaf chain and the
 * same stored normalised rows as uia_retrieval_ranks, so the same bits for the same two rows, whatever tile, lane, split or shape holds them (the paired
 * i2t listing is (img, txt), the t2i listing (txt, img): a product commutes bit for bit).
 * Row q of the outputs is the first K candidates under ONE total order: score descending by IEEE comparison (+0 == -0), equal scores by gallery index
 * ascending; a NaN score ranks below every non-NaN score, NaN scores among themselves by index ascending (a NaN query row lists 0 .. K-1 with NaN
 * scores; a NaN gallery row appears only when fewer than K others exist).  idx int32 [Q][K]: idx[q][r] is the gallery index of place r + 1;
 * score fp32 [Q][K] its s_qj.  Padding rows, columns and k are masked by index: a zero-padded column is never selectable.
 * splits: the number of gallery strips a row tile's work is cut into (grid = row tiles x splits, partial lists merged per row by a second kernel);
 * 0 takes uia_retrieval_topk_splits(Q, N), a pure host function (512 blocks aimed at, at most one strip per 128 gallery rows, 1 once the row tiles
 * alone fill the device); 1 .. 512 otherwise, and a value above the rule's is held to it.  The order is total, so the result does not depend on splits.
 * Everything is checked before anything is enqueued (non-zero, uia_last_error(), nothing written).  Asynchronous, deterministic (no atomics); writes
 * every element of idx and score.  ws: uia_retrieval_topk_workspace_bytes(Q, N, E, K) of scratch (the two normalised copies and the partial lists,
 * at most 512 x 128 x K entries; 0 for a shape outside the limits). */
size_t uia_retrieval_topk_workspace_bytes(int Q, int N, int E, int K);
int uia_retrieval_topk_splits(int Q, int N);
int uia_retrieval_topk(void* stream, int Q, int N, int E, int K, const float* queries, const float* gallery, int normalize, int splits, void* ws,
                       size_t ws_bytes, int32_t* idx, float* score);
/* Zero-shot classification scores of one batch of image features (the rule of the reference's src/models/metaclip/zero_shot.py:162-182 and
 * biomedclip/zero_shot.py:176-222), one launch.  img fp32 [N,E] and prompts fp32 [T,E], raw tower outputs, row-major contiguous; class_off a HOST
 * array int32 [C+1]: class c owns the prompt rows class_off[c] .. class_off[c+1]-1 (class_off[0] == 0, class_off[C] == T; ragged classes allowed).
 * Limits, checked before anything is enqueued (non-zero, uia_last_error(), nothing launched): 2 <= C <= 8, 1 <= prompts per class <= 32, T <= 256,
 * 1 <= E <= 4096, 1 <= N <= 2^24, ld >= C, row >= 0.  Every row is divided by its L2 norm with NO eps (x / x.norm()): a zero image row gives NaN logits
 * for that image, a zero prompt row NaN for its class in every image; NaN is never an index.  s[i,t] = 100 * <img_n[i], prm_n[t]> on the exact fp32
 * MFMA (a k-ordered fmaf chain from 0); logits[i,c] = the fp32 sum of s[i,t] over the class's prompts in prompt order, divided once by their count.
 * The bits of logits[i,:] depend only on row i of img and on prompts, never on N or on the row's place in the batch: any batching gives the same table.
 * Outputs: logits fp32, row i at logits + (row + i) * ld (a whole split lands in one buffer; only those N rows, C values each, are written);
 * probs fp32 [N,C] contiguous or NULL: softmax of the logits, log-sum-exp form evaluated in fp64 (finite for logits of +-100); img_n fp32 [N,E]
 * contiguous or NULL: the normalised image rows.  Asynchronous, deterministic (no atomics), no workspace. */
int uia_zero_shot_score(void* stream, int N, int T, int E, int C, const int32_t* class_off, const float* img, const float* prompts, float* logits, int64_t ld,
                        int64_t row, float* probs, float* img_n);
/* The exact ROC curve of a split, as torchmetrics ROC(task="binary", thresholds=None) returns it.  p1 fp32 [N], labels int64 [N] in {0,1}, perm int64 [N]:
 * the permutation that sorts p1 ascending (as for uia_binary_cls_stats); 1 <= N <= 2^24.  Outputs on the device: count int32 [1], fpr and tpr fp64 [N+1],
 * thr fp32 [N+1].  Point 0 is (0, 0, thr = 1.0); then one point per distinct score in descending order, fpr = #{neg : p1 >= thr} / #neg,
 * tpr = #{pos : p1 >= thr} / #pos (integer counts, one fp64 division each; the axis of an absent class is all zeros); count = distinct scores + 1, and
 * entries from count on are left as they were.  A label outside {0,1}, a perm entry outside [0,N) or a NaN score gives count = -1 and leaves the arrays
 * unwritten.  One workgroup, group ends compacted with a scan: deterministic, no atomics.  ws: uia_binary_roc_curve_workspace_bytes(N) of scratch. */
size_t uia_binary_roc_curve_workspace_bytes(int N);
int uia_binary_roc_curve(void* stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes, int32_t* count,
                         double* fpr, double* tpr, float* thr);

/* Training-time augmentation of a batch, one launch (the reference's src/datasets/{segmentation,classification}.py:14-156 on the device).  images fp32
 * [B,1,S,S] in [0,1] (4-byte aligned; 16-byte accesses where an image starts on 16 bytes), masks uint8 [B,1,S,S] or NULL (then out_masks is NULL too),
 * 1 <= B <= 65535, 8 <= S <= 1024.  programs: a HOST array int32 [B][14][4], every random decision already made: row 0 of an image is (n, with_mask,
 * 0, 0) with 0 <= n <= 13 (only n is read; the sampler notes there whether it drew for a batch with masks), rows 1 .. n are (opcode, p0, p1, p2), float parameters as float32 bit patterns: 0 identity, 1 autocontrast, 2 equalize,
 * 3 blur (p0 = sigma in [0.1, 2.5]), 4 contrast, 5 brightness, 6 sharpness (p0 = factor in [0, 4]), 7 posterize (p0 = bits, 1 .. 8), 8 solarize (p0 =
 * threshold, 0 .. 256), 9 crop (p0, p1, p2 = top row i, left column j, side; resized to S x S), 10 horizontal flip, 11 vertical flip.  The whole table is
 * checked before anything is enqueued (an unknown opcode, a parameter out of range, a crop leaving the image, n > 13: non-zero, nothing written); it is
 * then copied to the workspace with hipMemcpyAsync on `stream`, so a pinned table must stay as it is until that copy has run.
 * An image with n == 0 is copied bit for bit, and so is its mask.  Otherwise the image is quantised once to 8 bits (rint(255 x), clamped), run through
 * its ops as PIL 12.2 runs them on an "L" image (integer / fp32 / fp64 arithmetic restated exactly; the crop is PIL's two-pass fixed-point bilinear
 * resample) and written as q / 255; the mask bytes follow crop (PIL's nearest scaler) and flips.  The blur alone is this build's: the true separable
 * Gaussian, taps to ceil(4 sigma), replicated edges, fp32 sums in tap order, rounded half up.  out_images / out_masks must not overlap the inputs.
 * Asynchronous, deterministic (integer atomics only).  ws: uia_augment_workspace_bytes(B, S) of 16-byte aligned scratch (0 for a shape outside the
 * limits): the device copy of the table, two byte planes and one fp32 plane per image, two byte planes per mask. */
size_t uia_augment_workspace_bytes(int B, int S);
int uia_augment_batch(void* stream, int B, int S, const float* images, const uint8_t* masks, const int32_t* programs, void* ws, size_t ws_bytes,
                      float* out_images, uint8_t* out_masks);

/* The same launch on a device-resident set (the few-shot entries' training set, uploaded once): output b is made from row `src` of images [N,1,S,S],
 * where row 0 of output b in the table is (n, with_mask, src, 0) — the table format and its one host-to-device copy are those above.  src_dtype 0: the
 * resident images are fp32 and the result is uia_augment_batch's on the gathered rows.  src_dtype 1: they are uint8, the 8-bit plane itself (no
 * quantisation pass; an n == 0 row is written as (float)u / 255.0f): bit for bit uia_augment_batch on rows.float() / 255.  masks uint8 [N,1,S,S] or NULL.
 * A row may serve any number of outputs and B may exceed N.  Checked before anything is enqueued, beside everything uia_augment_batch checks: N >= 1,
 * src_dtype in {0, 1}, 0 <= src < N for every output, and the outputs ([B] rows) may not overlap the resident tensors ([N] rows).  Byte rows on 16 bytes
 * move 16 bytes per access, rows on 4 bytes a word, others single bytes.  ws: uia_augment_workspace_bytes(B, S) — sized by B, not N.  Asynchronous,
 * deterministic. */
int uia_augment_gather(void* stream, int N, int B, int S, int src_dtype, const void* images, const uint8_t* masks, const int32_t* programs, void* ws,
                       size_t ws_bytes, float* out_images, uint8_t* out_masks);

/* `Image.resize` of a batch of decoded images of different sizes, one launch, equal to Pillow 12.2 in every byte (csrc/resize.hip; the arithmetic
 * in plain Python: src/datasets/pil_resize.py).  src: B images back to back in one DEVICE byte buffer of src_bytes bytes (< 2^31), 8 bits per channel, C in
 * {1, 3} interleaved channels, at arbitrary byte offsets (read a byte at a time: no alignment is asked).  desc: a HOST array int32 [B][8], per image
 * (offset, H, W, mask_offset or -1, dst_h, dst_w, y0, x0): the H x W image at `offset` is resampled to dst_h x dst_w and the S x S window at (y0, x0)
 * of that result is written to out_images fp32 [B,C,S,S] (planar) as (float)q / 255.0f.  The square squash of the reference's supervised loaders is
 * dst_h = dst_w = S, y0 = x0 = 0; Resize(S) + CenterCrop(S) of its contrastive loader is the window form with C = 3.  Images: Pillow's two-pass
 * fixed-point resample with the antialiased bicubic filter (a = -0.5; float64 coefficients normalised in tap order and rounded to 22 bits,
 * clip8((2^21 + sum p k) >> 22), columns first with an 8-bit intermediate, a pass whose axis keeps its size skipped).  Masks: one byte per pixel, H x W, at
 * mask_offset; Pillow's nearest scaler (source index int(xo), xo = a / 2 stepped by a = in / dst in float64), written to out_masks uint8 [B,1,S,S] as
 * source byte != 0; an image without a mask gets zeros; out_masks may be NULL when no image has a mask.  Checked before anything is enqueued (non-zero,
 * nothing written, the image's index in uia_last_error()): 1 <= B <= 65535, 8 <= S <= 1024, C in {1, 3}, H, W >= 1, image and mask inside src,
 * 1 <= dst_h, dst_w <= 16384, the window inside dst, at most 129 taps per pixel on both axes (2 ceil(2 max(in / dst, 1)) + 1: a downscale of at most
 * 32x), out_masks given when an image has a mask, outputs that overlap neither src nor each other.  The descriptor is then copied to the workspace with
 * hipMemcpyAsync on `stream`, so a pinned descriptor must stay as it is until that copy has run.  Asynchronous, deterministic (no atomics).
 * ws: uia_resize_workspace_bytes(B) of 4-byte aligned scratch (0 for a B outside the limits): the device copy of the descriptor; the 8-bit
 * intermediate lives in LDS. */
size_t uia_resize_workspace_bytes(int B);
int uia_resize_batch(void* stream, int B, int C, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes, float* out_images,
                     uint8_t* out_masks);

/* uia_resize_batch for a batch that mixes gray and colour images, three planes out: the reference's contrastive loader (convert("RGB") when the mode
 * is not RGB, Resize(S, BICUBIC), CenterCrop(S), ToTensor) in one launch.  Word 3 of an image's descriptor is its CHANNEL COUNT, 1 or 3 (there are no
 * masks): (offset, H, W, channels, dst_h, dst_w, y0, x0).  out_images is fp32 [B,3,S,S]; a one-channel image is resampled once and its result written
 * to all three planes, which is Pillow's convert("RGB") of an "L" image followed by the resize (the channels run the same arithmetic).  Everything else
 * — the arithmetic, the limits, the checks made before anything is enqueued with the image's index in uia_last_error(), the workspace
 * (uia_resize_workspace_bytes(B)), the descriptor's asynchronous copy — is uia_resize_batch's; a channel count other than 1 or 3 is refused. */
int uia_resize_batch_rgb(void* stream, int B, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes, float* out_images);

/* The way back from a model's S x S logits to each image's own H x W: the inverse of uia_resize_batch's square squash, one launch per batch
 * (csrc/seg_native.hip).  logits fp32 [B,2,S,S], contiguous, 4-byte aligned.  src: the batch's ragged DEVICE byte buffer of src_bytes bytes (< 2^31) as
 * uia_resize_batch read it, gray bytes H_b x W_b back to back; NULL (src_bytes ignored) when no image asks for an overlay.  out: one DEVICE byte buffer
 * of out_bytes bytes (< 2^31).  desc: a HOST array int32 [B][8], per image (src_offset or -1, H, W, mask_out_offset, overlay_out_offset or -1, 0, 0, 0).
 * stats: DEVICE int32 [B][8].  Offsets are arbitrary bytes: no alignment is asked of src or out (4-byte stores are used where an address allows them,
 * decided inside the kernel).
 * For native pixel (y, x) of image b the two logit planes are sampled as torch.nn.functional.interpolate(size=(H, W), mode="bilinear",
 * align_corners=False) samples them, in fp32, every product and sum rounded once: scale_y = (float)S / H, sy = max(scale_y * (y + 0.5f) - 0.5f, 0),
 * y0 = (int)sy, y1 = min(y0 + 1, S - 1), ly = sy - y0, the same for x; per plane c the taps are combined rows first, then columns:
 * v_c[k] = (1 - ly) L_c[y0][k] + ly L_c[y1][k] for k = x0, x1, then u_c = (1 - lx) v_c[x0] + lx v_c[x1]; a tap whose weight is exactly 0 does not enter
 * (ly == 0: v_c[k] = L_c[y0][k]; lx == 0: u_c = v_c[x0]), so H = W = S gives the logits themselves.
 * p = 255 where argmax over (u_0, u_1) is class 1 by torch's rules (a tie, -0.0 against +0.0 included, goes to class 0; NaN is the maximum; NaN in
 * both goes to class 0), the prediction uia_seg_viz, uia_surface_distances and the Dice / IoU metrics use, else 0.
 * Outputs: the mask, H * W bytes of p at out + mask_out_offset, plain row-major; when src_offset and overlay_out_offset are both >= 0 the overlay,
 * H * W * 3 bytes (g, max(g, p), g) at out + overlay_out_offset with g the source byte at src_offset + y * W + x (uia_seg_viz's overlay without a ground
 * truth); stats[b] = (foreground pixel count, ymin, xmin, ymax, xmax, 0, 0, 0), (0, INT_MAX, INT_MAX, -1, -1, 0, 0, 0) for an empty mask: the call sets
 * that initial value itself on `stream`.  Every byte of the ranges and of stats is written, nothing beside them.
 * Checked before anything is enqueued (non-zero, nothing written, the image's index in uia_last_error()): 1 <= B <= 65535, 8 <= S <= 1024,
 * 1 <= H, W <= 16384, null logits / desc / out / ws / stats, a null src when an image asks for an overlay, offsets below -1, a source image, mask or
 * overlay that leaves its buffer, output ranges that overlap each other, src, logits, stats or the workspace, a non-zero reserved descriptor word.
 * The descriptor is then copied to the workspace with hipMemcpyAsync on `stream`, so a pinned descriptor must stay as it is until that copy has run.
 * Asynchronous, deterministic (integer atomics only).  ws: uia_seg_native_workspace_bytes(B) of 4-byte aligned scratch (0 for a B outside the
 * limits): the device copy of the descriptor. */
size_t uia_seg_native_workspace_bytes(int B);
int uia_seg_predict_native(void* stream, int B, int S, const float* logits, const uint8_t* src, size_t src_bytes, const int32_t* desc, uint8_t* out,
                           size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats);

/* uia_seg_predict_native for an ensemble of K members (checkpoints, flips of the model's input, or both), with a threshold the caller sets, a
 * probability map and a spread map: one launch per batch (csrc/seg_native_ens.hip).  logits fp32 [K][B][2][S][S], contiguous, 4-byte aligned,
 * 1 <= K <= 16.  flips holds two bits per member: bit 2k says that member k's logits are of the horizontally flipped S x S input, bit 2k + 1 the same
 * for a vertical flip; the kernel reads member k's planes as L'_c[y][x] = L_c[fy ? S - 1 - y : y][fx ? S - 1 - x : x]; bits at or above 2 K must be
 * zero.  threshold: a finite float with 0 < threshold < 1.  src, out, stats, the limits on B, S, H, W and the buffer sizes: uia_seg_predict_native's.
 * desc: a HOST array int32 [B][8], per image (src_offset or -1, H, W, mask_out_offset, overlay_out_offset or -1, probability_out_offset or -1,
 * spread_out_offset or -1, 0); offsets are arbitrary bytes, no alignment is asked.  sums: DEVICE uint64 [B][2], 8-byte aligned, or NULL.
 * Per native pixel and member k, u_0 and u_1 are computed from L' exactly as uia_seg_predict_native computes them (the same coordinates, rows first,
 * then columns, a tap of weight exactly 0 left out, every product and sum rounded once in fp32); z_k = u_1 - u_0, p_k = 1 / (1 + expf(-z_k)) with an
 * IEEE division; P = (p_0 + ... + p_{K-1}) / K, summed in member order in fp32.
 * Outputs: the mask, 255 where P > threshold (strictly), else 0; the overlay (g, max(g, mask), g) as uia_seg_predict_native's; at the probability
 * offset H * W bytes q = (uint8)(255 P + 0.5f); at the spread offset H * W bytes r = (uint8)(255 (max_k p_k - min_k p_k) + 0.5f), 0 at K = 1.  A pixel
 * where any z_k is NaN gets mask 0, q = 0, r = 255; infinite logits follow IEEE (z = +inf gives p = 1, -inf gives 0, inf - inf is NaN).
 * stats[b] = (foreground count, ymin, xmin, ymax, xmax, 0, 0, 0) with uia_seg_predict_native's empty value, set by the call itself, so
 * uia_mask_components reads the result unchanged.  sums[b] = (sum of q over the pixels whose mask byte this launch wrote as 255, sum of r over all
 * pixels), zeroed by the call and accumulated with 64-bit integer atomics, computed whether or not the map is stored.
 * Asynchronous, deterministic (integer atomics only: two calls give identical bytes).  Every byte of the requested ranges, of stats and of sums is
 * written, nothing beside them.
 * Checked before anything is enqueued (non-zero, nothing written, the image's index in uia_last_error()): everything uia_seg_predict_native checks,
 * K outside 1 .. 16, stray flip bits, a threshold outside (0, 1) or NaN, a misaligned sums, a probability or spread map that leaves `out` or overlaps
 * any other range, src, logits, stats, sums or the workspace, a non-zero reserved word (word 7).  The descriptor is then copied to the workspace with
 * hipMemcpyAsync on `stream`, so a pinned descriptor must stay as it is until that copy has run.  ws: uia_seg_native_ens_workspace_bytes(B) of 4-byte
 * aligned scratch (0 for a B outside the limits): the device copy of the descriptor. */
size_t uia_seg_native_ens_workspace_bytes(int B);
int uia_seg_predict_native_ens(void* stream, int K, int B, int S, const float* logits, uint32_t flips, float threshold, const uint8_t* src, size_t src_bytes,
                               const int32_t* desc, uint8_t* out, size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats, uint64_t* sums);

/* Connected-component filtering of native-size masks where they lie, and one row per kept lesion (csrc/components.hip).  buf: one DEVICE byte buffer of
 * buf_bytes bytes (< 2^31), in the prediction path the `out` buffer of uia_seg_predict_native as it returned.  desc: a HOST array int32 [B][8], per image
 * (mask_offset, H, W, overlay_offset or -1, min_area, keep, connectivity, 0); offsets are arbitrary bytes.  A mask byte != 0 is foreground; components
 * are 4- or 8-connected per `connectivity`; a component's first pixel is its smallest raster index y * W + x; components are ordered by area, largest
 * first, equal areas by smaller first pixel first; a component is kept when area >= min_area and (keep == 0 or its position in that order < keep).
 * Written: every pixel of a component that is not kept gets mask byte 0 and, with an overlay, overlay byte[1] = byte[0] (the overlay is
 * (g, max(g, p), g)); kept pixels and background keep their bytes.  stats: DEVICE int32 [B][8] = (foreground after, ymin, xmin, ymax, xmax after,
 * components found, components kept, foreground before), the box of an empty result (INT_MAX, INT_MAX, -1, -1): words 0-4 mean what they mean in
 * uia_seg_predict_native.  list: DEVICE int32 [B][max_list][8], 0 <= max_list <= 32 (NULL allowed at 0): the first max_list kept components in that
 * order, each (area, ymin, xmin, ymax, xmax, first pixel, floor(sum y / area), floor(sum x / area)) with 64-bit sums; unused rows are zeros.  Every
 * word of stats and list is written; nothing beside them, the mask bytes and the overlays' green bytes is touched.
 * Checked before anything is enqueued (non-zero, nothing written, the image's index in uia_last_error()): 1 <= B <= 65535, 1 <= H, W <= 16384, null
 * buf / desc / ws / stats, a null list with max_list > 0, max_list outside 0 .. 32, a connectivity other than 4 or 8, a negative min_area or keep, a
 * non-zero reserved word, a mask or overlay that leaves buf, ranges that overlap each other, stats, list or the workspace, a workspace below
 * uia_mask_components_workspace_bytes(B, pixels) with pixels = the sum of H * W over the batch (0 for arguments outside the limits; 8-byte aligned;
 * 8 bytes per pixel and about 3.4 KiB per image).  The descriptor is then copied to the workspace with hipMemcpyAsync on `stream`, so a pinned
 * descriptor must stay as it is until that copy has run.  Asynchronous, no host synchronisation; integer atomics only, so two calls on equal input
 * give identical bytes whatever the scheduling. */
size_t uia_mask_components_workspace_bytes(int B, int64_t pixels);
int uia_mask_components(void* stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats, int32_t* list,
                        int max_list);

/* Disk closing, hole filling and disk opening of native-size masks where they lie (csrc/morphology.hip).  buf: one DEVICE byte buffer of buf_bytes bytes
 * (< 2^31), in the prediction path the `out` buffer of uia_seg_predict_native / _ens as it returned.  desc: a HOST array int32 [B][8], per image
 * (mask_offset, H, W, overlay_offset or -1, r_close, r_open, hole_area, hole_connectivity); offsets are arbitrary bytes.  A mask byte != 0 is
 * foreground.  With D the image's pixel grid and disk(r) = {(dy, dx) : dy^2 + dx^2 <= r^2}:  dilate_r(X) = {p in D : some q in X with p - q in disk(r)}
 * (the exact squared Euclidean distance from p to X is <= r^2; pixels outside the image contribute nothing);  erode_r(X) = D \ dilate_r(D \ X) (only
 * background INSIDE the image erodes: scipy's binary_dilation(border_value=0) / binary_erosion(border_value=1) with the disk, so closing is extensive,
 * opening anti-extensive, both idempotent);  a hole is a connected component of the background under hole_connectivity (4 or 8) with no pixel in the
 * first or last row or column of the image; it is filled when hole_area == -1 (any size) or its area <= hole_area; hole_area == 0 fills nothing.
 * Per image, in this order: X1 = erode_rc(dilate_rc(X0)), X2 = X1 + the filled holes of X1, X3 = dilate_ro(erode_ro(X2)); a radius of 0 is the identity.
 * Written: a pixel of X3 \ X0 gets mask byte 255 and, with an overlay, overlay byte[1] = 255; a pixel of X0 \ X3 gets mask byte 0 and overlay byte[1] =
 * byte[0]; every other byte keeps its value, bytes other than 255 included.  stats: DEVICE int32 [B][8] = (foreground after, ymin, xmin, ymax, xmax after,
 * pixels added, pixels removed, foreground before), the box of an empty result (INT_MAX, INT_MAX, -1, -1): words 0-4 mean what they mean in
 * uia_seg_predict_native.  Every word of stats is written; nothing beside stats, the mask bytes and the overlays' green bytes is touched.
 * Checked before anything is enqueued (non-zero, nothing written, the image's index in uia_last_error()): 1 <= B <= 65535, 1 <= H, W <= 16384, null
 * buf / desc / ws / stats, a radius outside 0 .. 64, a hole_area below -1, a hole_connectivity other than 4 or 8 (even where hole_area is 0), an offset
 * below -1 or a mask offset of -1, a mask or overlay that leaves buf, ranges that overlap each other, stats or the workspace, a workspace below
 * uia_mask_morphology_workspace_bytes(B, pixels) with pixels = the sum of H * W over the batch (0 for arguments outside the limits; 8-byte aligned;
 * 10 bytes per pixel — two byte planes, a label and an area word — and about 40 bytes per image).  The descriptor is then copied to the workspace with
 * hipMemcpyAsync on `stream`, so a pinned descriptor must stay as it is until that copy has run.  Only the launches some image needs are enqueued.
 * Asynchronous, no host synchronisation; integer atomics only, so two calls on equal input give identical bytes whatever the scheduling. */
size_t uia_mask_morphology_workspace_bytes(int B, int64_t pixels);
int uia_mask_morphology(void* stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats);

/* ---------------------------------------------------------------------------------------------
 * Layout helpers around the GEMMs. */
int uia_cast(void* stream, int dtype, size_t n, const float* src, void* dst, float scale);          /* dst = T(scale*src) */
int uia_transpose_cast(void* stream, int dtype, int rows, int cols, const float* src, void* dst);   /* dst[c][r] = T(src[r][c]) */

/* All GEMM-operand forms of a set of small trainable fp32 matrices in ONE launch (the adapter weights after an optimiser step):
 * for matrix i (src [rows][cols] fp32), any non-null of
 *     row    [rows][cols]            T copy                         (weight [N = rows][K = cols] of y = x·Wᵀ)
 *     row_kb [cols/g][rows][g]       its K-blocked twin, g = 64 bytes of T elements (cols % g == 0)
 *     tr     [cols][rows]            T transpose                    (the dgrad weight)
 *     tr_kb  [rows/g][cols][g]       K-blocked twin of the transpose (rows % g == 0)
 * The descriptor table lives in DEVICE memory (the caller uploads it once and re-uses it every step).  Replaces, per matrix and
 * step, the reference's implicit autocast casts (torch.autocast around F.linear: /root/reference/src/models/biomedclip/finetune.py:277). */
typedef struct uia_pack_desc {
    const float* src;
    void* row;
    void* row_kb;
    void* tr;
    void* tr_kb;
    int32_t rows, cols;
    /* The destinations may be LARGER than the source: rows_pad x cols_pad (0 = rows / cols).  Only the source's elements are written, so
     * destinations zeroed once stay zero-padded — a LoRA factor [r, in] / [out, r] (r = 16) becomes the 64-wide GEMM operand in the same
     * launch that casts it.  scale (0 = 1) multiplies every element before the cast (lora.py:87's scaling folded into B). */
    int32_t rows_pad, cols_pad;
    float scale;
    int32_t reserved_;
} uia_pack_desc;
int uia_pack_weights(void* stream, int dtype, int n, const uia_pack_desc* descs_device, int max_elems);
int uia_im2col(void* stream, int dtype, int B, int C, int H, int W, int P, const float* img, void* out); /* model.py:221,234 */
/* same for any patch size (P need not be a multiple of 4), rows padded with zeros to ldo >= C*P*P columns (ViT-L/14: 588 -> 640) */
int uia_im2col_padded(void* stream, int dtype, int B, int C, int H, int W, int P, const float* img, void* cols, int64_t ldo);
int uia_fill_cls(void* stream, int B, int N, int D, const float* cls, const float* pos0, float* x);   /* model.py:237-245 */
/* table [vocab, D], pos [max_pos, D]: L > max_pos is rejected; an id outside [0, vocab) (nn.Embedding raises for it) yields a NaN row,
 * which trips the training loops' non-finite-loss check instead of reading past the table */
int uia_embed(void* stream, int rows, int L, int D, int vocab, int max_pos, const int64_t* ids, const float* table, const float* pos,
              const float* type0, float* out);                                                          /* model.py:362-364 */
/* un-padded text tower (opt-in): rows are the valid tokens only; pos_idx[r] is the token's position inside its caption */
int uia_embed_packed(void* stream, int rows, int D, int vocab, int max_pos, const int64_t* ids, const int64_t* pos_idx, const float* table,
                     const float* pos, const float* type0, float* out);
/* nn.Embedding backward for --method full --tune_text_encoder: dtable[ids[r]] += dx[r] (fp32 atomics into a caller-zeroed table);
 * rows whose id equals pad_id are skipped (padding_idx). */
int uia_embed_bwd(void* stream, int rows, int D, int vocab, const int64_t* ids, const float* dx, float* dtable, int64_t pad_id);
int uia_gather_rows(void* stream, int n, int D, const float* src, const int64_t* idx, float* dst);  /* model.py:372 */
/* dst[r] = src[r·src_stride_bytes .. + row_bytes) for r < rows, dst compact: every stride-th row of a tensor of any element type (the CLS rows of a
 * saved activation).  row_bytes, src_stride_bytes and both pointers are whole 16-byte units. */
int uia_copy_rows(void* stream, int rows, int64_t row_bytes, const void* src, int64_t src_stride_bytes, void* dst);
/* dst[r·D + c] = the fp32 value of element (r·stride_rows, c) of a three-byte tensor, r < rows: float bits = (hi bits << 16) + (lo << 8).  hi: the bf16 plane,
 * row-major (hi_kb_rows = 0, rows ldhi elements apart) or K-blocked with hi_kb_rows rows (element (row, c) at hi[((c/32)·hi_kb_rows + row)·32 + c%32], D a
 * multiple of 32); lo: the int8 plane, row-major, rows ldlo apart.  The CLS rows of a residual stream that travels as three bytes per element. */
int uia_rows3_to_f32(void* stream, int rows, int D, int64_t stride_rows, const void* hi, int64_t ldhi, int64_t hi_kb_rows, const int8_t* lo, int64_t ldlo, float* dst);
/* dst = (accumulate ? dst : 0) + src*keep/(1-p), keep from the counter hash of (seed, index): LoRA input dropout
 * (src/adapters/lora.py:82-83) and its backward (same seed). */
int uia_dropout(void* stream, int dtype, size_t n, const void* src, void* dst, float p, uint64_t seed, int accumulate);
/* out[N] += column sums of A[M,N] (bias gradients; LinearLoRA biases train: SURVEY Appendix C-4). */
int uia_colsum(void* stream, int dtype, int M, int N, const void* A, int64_t lda, float* out);

/* ---------------------------------------------------------------------------------------------
 * CLIPSeg decoder pieces (src/third_party/openai_clip/clipseg_adapter.py:73-98 → transformers CLIPSegDecoder [third-party],
 * SURVEY Appendix A.3).  Its Linear / convolution contractions are uia_gemm + uia_wgrad; uia_attn_* accepts head dim 16 / 32
 * (plain-VALU path) besides 64.  These are the remaining stages; the decoder is trainable, so all have backwards. */
int uia_layernorm_bwd_affine(void* stream, int dtype, int M, int D, const void* dy, const float* x, const float* gamma, float eps,
                             const float* dres, float* dx32, float* g_gamma, float* g_beta);   /* dx and += dgamma, dbeta */
int uia_film_fwd(void* stream, int B, int N, int C, const float* x, const float* mul, const float* add, float* y);   /* y = mul[b]*x + add[b] */
int uia_film_bwd(void* stream, int B, int N, int C, const float* dy, const float* x, const float* mul, float* dx, float* dmul, float* dadd);
/* 3x3 / pad-1 patches of the token grid: cols[(b*h*w+p)][(ky*3+kx)*C + c] = x[b][tok_off + nbr][c]; col2im is its adjoint
 * (rows < tok_off of dx are zeroed). */
int uia_im2col3x3(void* stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const float* x, void* cols);
int uia_col2im3x3(void* stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const void* dcols, float* dx);
/* two stacked kernel=stride transposed convolutions leave [B*h*w*k1*k1, >=k2*k2]; unshuffle writes logits [B, h*k1*k2, w*k1*k2] (+bias). */
int uia_unshuffle(void* stream, int dtype, int B, int h, int w, int k1, int k2, const void* tmp, int64_t ld, float bias, float* out);
int uia_shuffle(void* stream, int dtype, int B, int h, int w, int k1, int k2, const float* dout, void* dtmp, int64_t ld);
/* out = dy * act'(.) where y is the stored POST-activation for ReLU and the stored PRE-activation for GELU / QuickGELU */
int uia_act_bwd(void* stream, int dtype, size_t n, const void* dy, const void* y, int act, void* out);

/* ---------------------------------------------------------------------------------------------
 * Symmetric InfoNCE (src/losses/losses.py:23-47), forward + gradients of both feature matrices, fp32.
 * loss (1 float, device) is overwritten; dimg/dtxt (both or neither) receive grad_scale * dLoss/dfeat.
 * workspace: uia_infonce_workspace_bytes(B, E). */
size_t uia_infonce_workspace_bytes(int B, int E);
int uia_infonce_fwd_bwd(void* stream, int B, int E, const float* img, const float* txt, float inv_temp, float grad_scale,
                        float* loss, float* dimg, float* dtxt, void* workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * One optimiser update on the flat fp32 adapter buffer: clip_grad_norm_(max_norm) + AdamW
 * (src/models/biomedclip/finetune.py:244-249,297-302).  g is read as grad_scale*g (1/world after the
 * all-reduce SUM).  ws2: 2 floats of device scratch; ws2[0] returns the squared gradient norm. */
int uia_adamw_clip_step(void* stream, size_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float max_norm, int step, float grad_scale, float* ws2);

/* Guarded forms for loops that never read the loss on the host (round 5).  The reference decides per micro-batch on the host
 * (src/models/biomedclip/finetune.py:281-285: a non-finite loss skips the backward AND the update check of that iteration);
 * these take the same two decisions on the device.
 *   uia_grad_accum_guarded: mb[0..n) is the staging buffer one micro-batch's backward wrote; when *loss is finite it is added to
 *     acc[0..n), mb is zeroed either way.  acc has n + 4 floats: acc[n] = 0 (finite) / 1 (not) for THIS micro-batch — all-reduced
 *     with the gradients it becomes "ranks whose boundary micro-batch was non-finite".  stats[0] += loss (finite only);
 *     ctl (4 x int32): [0] updates applied, [1] micro-batches accumulated, [2] micro-batches skipped, [3] updates skipped;
 *     ok_log (optional): ok_log[log_index] = 1 / 0 for the host's end-of-epoch log.
 *   uia_adamw_clip_step_guarded: one clip + AdamW update from acc when acc[n] == 0, acc zeroed in the same pass (zero_grad);
 *     otherwise nothing but acc *= skip_scale (1/world under data parallelism: the summed buffer becomes this rank's share again).
 *     The update index t = ctl[0] lives on the device: lr = lr_min + (lr - lr_min)(1 + cos(pi t / t_max))/2 (CosineAnnealingLR,
 *     finetune.py:255; t_max = 0: constant lr) and the bias corrections use step t + 1, so a skipped update does not advance
 *     the schedule.  ws8: 8 floats of device scratch; ws8[0] returns the squared gradient norm, ws8[1] whether the update ran. */
int uia_grad_accum_guarded(void* stream, size_t n, float* acc, float* mb, const float* loss, float* stats, int32_t* ctl, uint8_t* ok_log, int64_t log_index);
int uia_adamw_clip_step_guarded(void* stream, size_t n, float* p, float* acc, float* m, float* v, float lr, float lr_min, int t_max, float beta1, float beta2,
                                float eps, float weight_decay, float max_norm, float grad_scale, float skip_scale, float* ws8, int32_t* ctl);

/* ---------------------------------------------------------------------------------------------
 * DINOv2 UNet decoder (dino/dinov2.py:130-260 [third-party]): convolutions, BatchNorm + ReLU and resampling on NHWC activations
 * (channels innermost).  Fixed reduction orders throughout: two identical calls give identical bits.
 *
 * uia_conv_igemm: implicit GEMM y[m][n] = Σ_k w[n][k]·x[m][k] (+ bias), x gathered per tap from the activation (no im2col).
 *   UIA_CONV3      3x3, pad 1, stride 1 on a B×H×W grid.  Sources x1 [B,H,W,C1] and x2 [B,H,W,C2] (C2 = 0: none) are the channel
 *                  halves of one input; w [N][9][C1+C2]; channels [0, N1) go to y1 [B,H,W,N1], [N1, N) to y2 [B,H,W,N−N1].  The data
 *                  gradient is the same call on dy with the flipped, transposed weight.
 *   UIA_CONVT_FWD  ConvTranspose2d k=2 s=2 of x1 [B,H,W,C1]: w [4·Cout][C1] (row (2·di+dj)·Cout + o), N = 4·Cout, N1 = N, bias [Cout];
 *                  y1 [B,2H,2W,Cout].
 *   UIA_CONVT_BWD  its data gradient: x1 = dy [B,2H,2W,C1 = Cout], w [N = Cin][4][Cout], y1 = dx [B,H,W,Cin], N1 = N.
 *   UIA_CONV1      Conv2d k=1 of x1 [B,H,W,C1] (the baseline UNet's conv1x1, src/third_party/unet.py:42): w [N][C1], N1 = N, y1 [B,H,W,N].
 *                  The data gradient is the same call on dy with the transposed weight.
 *   bias: fp32 or null.  MFMA path when C1, C2 % 8 == 0, N, N1 (and Cout) % 4 == 0 and operands 16-byte aligned; a direct path otherwise.
 *   K = taps·(C1+C2) need not be a multiple of the 32-wide K step: the last step is zero-filled.  Shapes with C1, C2 % 32 == 0 run the
 *   kernel they always ran (same bits).
 * uia_conv_wgrad: fp32 weight gradient over the B×H×W pixels in uia_conv_wgrad_splits(...) pixel ranges added in range order.
 *   UIA_CONV3      dw [N][9·(C1+C2)] from x1 / x2 and dy [B,H,W,N].
 *   UIA_CONVT_FWD  dw [4·N][C1] from x1 [B,H,W,C1] and dy [B,2H,2W,N] (N = Cout).
 *   UIA_CONV1      dw [N][C1] from x1 [B,H,W,C1] and dy [B,H,W,N].
 *   ws: splits·rows·cols floats when splits > 1 (may be null otherwise).  MFMA path when C1, C2 % 8 == 0 and N % 8 == 0.
 * uia_conv_igemm_form / uia_conv_wgrad_form: 1 when the matrix-core kernel is taken for 16-byte-aligned operands, 0 for the direct
 *   kernel (pure functions of the shape, callable without a GPU; the launchers decide by them).  They tell which of the baseline UNet's
 *   layers (src/third_party/unet.py:5-111, init_channels = 16) leave the direct kernel: all but the 3-channel input and num_classes output. */
enum { UIA_CONV3 = 0, UIA_CONVT_FWD = 1, UIA_CONVT_BWD = 2, UIA_CONV1 = 3 };
#define UIA_WGRAD_MAX_SPLITS 64            /* MFMA path, C1 and C2 multiples of 32 (N % 8) */
#define UIA_WGRAD_MAX_NARROW_SPLITS 512    /* MFMA path, C1 or C2 not a multiple of 32 (few tiles, the most pixels) */
#define UIA_WGRAD_MAX_DIRECT_SPLITS 1024    /* direct path (few channels) */
int uia_conv_igemm(void* stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N, int N1,
                   const void* w, const float* bias, void* y1, void* y2);
int uia_conv_wgrad_splits(int mode, int B, int H, int W, int C1, int C2, int N);
int uia_conv_igemm_form(int mode, int C1, int C2, int N, int N1);
int uia_conv_wgrad_form(int mode, int C1, int C2, int N);
int uia_conv_wgrad(void* stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N, const void* dy,
                   float* ws, float* dw);
/* BatchNorm2d (+ ReLU when relu != 0) on y [M = B·H·W, C] (dtype elements), fp32 parameters and buffers.
 *   training: batch mean and biased variance; mean / invstd saved for the backward, running_mean / running_var updated with the unbiased
 *   variance (momentum), *num_batches_tracked += 1 (either buffer pointer may be null: no update).  eval: the running statistics.
 *   scale / shift [C] receive the folded affine, out = act(y·scale + shift).  ws: UIA_BN_SLICES·C·3 floats.
 * uia_bn_relu_bwd: dy from dout through ReLU and the training-mode statistics; dgamma = Σdz·x̂, dbeta = Σdz (overwritten).
 * uia_colsum_ordered: out[c] = Σ_m y[m][c] (fp32; the convs' bias gradients).  ws: UIA_BN_SLICES·C·3 floats. */
#define UIA_BN_SLICES 256
int uia_bn_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const float* gamma, const float* beta, float* running_mean,
               float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean, float* invstd, float* scale,
               float* shift, int relu, void* out);
int uia_bn_relu_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                    const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy);
int uia_colsum_ordered(void* stream, int dtype, int64_t M, int C, const void* y, float* ws, float* out);
/* BatchNorm2d + LeakyReLU(slope) + Dropout(drop_p) of the baseline UNet's ConvBlock (src/third_party/unet.py:10-18), on the arguments of
 * uia_bn_fwd / uia_bn_relu_bwd:  out = leaky(z)·keep/(1−drop_p), z = y·scale + shift, leaky(z) = z > 0 ? z : slope·z.
 *   Statistics, running buffers and scale / shift are exactly uia_bn_fwd's.  keep: keep_mask (uint8 [M, C]) when non-null, else, when
 *   drop_p > 0, the counter hash of (seed, flat element index / 8), the generator of uia_dropout (needs M·C % 8 == 0).  No dropout when
 *   drop_p == 0 or training == 0.  uia_bn_act_bwd: dz = dout·keep/(1−drop_p)·(z > 0 ? 1 : slope) (z == 0 takes the slope), then as
 *   uia_bn_relu_bwd.  slope = 0, drop_p = 0 gives uia_bn_fwd(relu = 1) bit for bit. */
int uia_bn_act_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean, float* invstd, float* scale,
                   float* shift, float slope, void* out, float drop_p, uint64_t seed, const uint8_t* keep_mask);
int uia_bn_act_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                   const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, float slope,
                   float drop_p, uint64_t seed, const uint8_t* keep_mask);
/* nn.MaxPool2d(2) of the baseline UNet's DownBlock (src/third_party/unet.py:29) on NHWC x [B,H,W,C] -> y [B,H/2,W/2,C] (floor: a trailing
 *   odd row / column is ignored).  Backward: the argmax is recomputed from x (ties to the first maximum in the order (0,0), (0,1), (1,0),
 *   (1,1), as PyTorch) and every element of dx [B,H,W,C] is written (zeros off the argmax and in the trailing row / column): no atomics,
 *   no memset.  H < 2 or W < 2 is refused. */
int uia_maxpool2_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, void* y);
int uia_maxpool2_bwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, const void* dy, void* dx);
/* uia_upsample_ac: bilinear, align_corners=True, integer factor f on NHWC: forward in [B,H,W,C] -> out [B,fH,fW,C]; backward (gather,
 *   no atomics) in = dout [B,fH,fW,C] -> out = dx [B,H,W,C].
 * uia_resize_aa: F.interpolate(bicubic, antialias=True, align_corners=False) from NHWC x [B,Hi,Wi,C] (dtype) to NCHW fp32 out
 *   [B,C,Ho,Wo] through tmp (fp32 [B,C,Hi,Wo]); backward: dout fp32 NCHW -> dx NHWC (dtype).  Downscale at most 3x. */
int uia_upsample_ac(void* stream, int dtype, int backward, int B, int H, int W, int C, int f, const void* in, void* out);
int uia_resize_aa(void* stream, int dtype, int backward, int B, int C, int Hi, int Wi, int Ho, int Wo, const void* x, float* tmp, float* out,
                  const float* dout, void* dx);

/* ---------------------------------------------------------------------------------------------
 * ResNet classification baseline (src/third_party/resnet.py): what a CNN other than a UNet needs, under the conventions of the section
 * above (NHWC, bf16 / fp32, fixed reduction orders, no float atomics, no memset: two identical calls give identical bits).
 *
 * uia_conv_strided: Conv2d(k, stride s, padding k/2, bias=False), k in {1, 3, 7}, s in {1, 2}, of x [B,H,W,C] with N output channels on the
 *   output grid Ho×Wo, Ho = (H − 1)/s + 1 (floor; odd and even H, W).  H, W and C always name the conv's INPUT, N its output.
 *   dgrad = 0  forward: x [B,H,W,C], w [N][k²·C] (column (ky·k + kx)·C + c) -> y [B,Ho,Wo,N].
 *   dgrad = 1  data gradient: x = dy [B,Ho,Wo,N], w [C][k²·N] (column (ky·k + kx)·N + n, taps not flipped) -> y = dx [B,H,W,C]: input pixel
 *              (y, x) takes tap (ky, kx) where y + k/2 − ky and x + k/2 − kx are divisible by s and the quotient lies in Ho×Wo.  Every
 *              tap runs; the invalid ones contribute zeros.
 *   MFMA path (the 64×128 tile of uia_conv_igemm) when C % 8 == 0, N % 8 == 0 and the operands are 16-byte aligned; a direct kernel otherwise.
 * uia_conv_strided_wgrad: fp32 dw [N][k²·C] from x [B,H,W,C] and dy [B,Ho,Wo,N] over the B·Ho·Wo output pixels, in
 *   uia_conv_strided_wgrad_splits(...) pixel ranges added in range order (the rule of uia_conv_wgrad_splits, the narrow-channel cap
 *   included).  ws: splits·N·k²·C floats when splits > 1.
 * uia_conv_strided_form / uia_conv_strided_wgrad_form: 1 when the matrix-core kernel is taken for 16-byte-aligned operands, else 0 (pure
 *   functions of the shape, callable without a GPU; the launchers decide by them).  Any other k or s is refused by the launchers.
 * The 7×7 stem (3 -> 64) runs on the MFMA path with 8 input channels, channels 3..7 zero: uia_nchw_to_nhwc packs the image and the weight. */
int uia_conv_strided(void* stream, int dtype, int dgrad, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* w, void* y);
int uia_conv_strided_wgrad_splits(int B, int H, int W, int C, int k, int s, int N);
int uia_conv_strided_form(int dgrad, int C, int N, int k, int s);
int uia_conv_strided_wgrad_form(int C, int N, int k, int s);
int uia_conv_strided_wgrad(void* stream, int dtype, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* dy, float* ws,
                           float* dw);
/* nn.MaxPool2d(kernel 3, stride 2, padding 1) on NHWC x [B,H,W,C] -> y [B,Ho,Wo,C], Ho = (H − 1)/2 + 1.  The padding is −inf, not 0: an
 *   all-negative window returns its maximum.  Backward: a gather with no atomics; each input pixel recomputes the argmax of the at most
 *   four windows that cover it (ties to the first maximum in row-major window order, as PyTorch), adds dy of the windows it wins in window
 *   order (fp32, rounded once) and writes every element of dx [B,H,W,C].  16-byte accesses when the channel count and the pointers allow,
 *   a scalar form otherwise.  Inputs are finite: the ordering of NaN is not part of the contract. */
int uia_maxpool3s2_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, void* y);
int uia_maxpool3s2_bwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, const void* dy, void* dx);
/* BatchNorm2d + residual add + ReLU, out = relu(y·scale + shift + r), on the arguments of uia_bn_fwd / uia_bn_relu_bwd.  Statistics, running
 *   buffers and scale / shift are exactly uia_bn_fwd's; r [M, C] (dtype) may be null, and then the result is uia_bn_fwd(relu = 1) bit for bit.
 *   uia_bn_add_relu_bwd takes the forward's out instead of scale / shift: dz = dout·[out > 0] (out == 0 takes 0), dr = dz (its own tensor,
 *   may be null), then the training-mode BatchNorm backward of uia_bn_relu_bwd on dz.  ws: UIA_BN_SLICES·C·3 floats.
 *   The downsample branch's BatchNorm without activation is uia_bn_act_fwd / uia_bn_act_bwd with slope = 1, drop_p = 0. */
int uia_bn_add_relu_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const void* r, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean,
                        float* invstd, float* scale, float* shift, void* out);
int uia_bn_add_relu_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* out, const void* dout, const float* mean,
                        const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, void* dr);
/* Global average pool of NHWC x [B,H,W,C] (dtype) -> pooled [B,C] fp32: the H·W pixels added in pixel order in fp32, divided once; one
 *   launch.  Backward: dx[b,y,x,c] = dout[b,c]/(H·W) (dtype), one launch. */
int uia_avgpool_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, float* pooled);
int uia_avgpool_bwd(void* stream, int dtype, int B, int H, int W, int C, const float* dout, void* dx);
/* Layout helper: fp32 NCHW x [B,Cin,H,W] -> NHWC out [B,H,W,Cout] (dtype).  Output channel c < rep copies input channel c (Cin == 1: input
 *   channel 0 for every c < rep, the widening of a one-channel batch); channels rep..Cout−1 are zero.  The stem's image (rep 3, Cout 8)
 *   and its weight [64,3,7,7] -> [64][49][8] (B = 64, H = W = 7) both pass through it.
 * uia_add2: out = a + b element-wise (fp32 sum rounded once; out may alias a or b): the sum of a block's two input gradients. */
int uia_nchw_to_nhwc(void* stream, int dtype, int B, int Cin, int H, int W, int Cout, int rep, const float* x, void* out);
int uia_add2(void* stream, int dtype, int64_t n, const void* a, const void* b, void* out);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel exchange (new: the reference is single-process, finetune.py:287-302 accumulates
 * instead).  RCCL all-reduce on the caller's stream; the unique id travels through the host.
 * Every RCCL failure is reported as "rank r/world: <call> failed: <reason>" through uia_last_error(). */
int uia_comm_unique_id_bytes(void);
int uia_comm_get_unique_id(void* out, int bytes);
int uia_comm_init(int rank, int world, const void* unique_id, int bytes);
int uia_comm_world(void);
int uia_comm_initialised(void);   /* 1 once uia_comm_init succeeded (a one-rank communicator is valid: its all-reduce is the identity) */
int uia_allreduce_sum(void* stream, int dtype, void* buf, size_t n);
/* opt-in global-batch contrastive loss: recv[r*n_per_rank ...] = rank r's send buffer (RCCL all-gather). */
int uia_allgather(void* stream, int dtype, const void* send, void* recv, size_t n_per_rank);
int uia_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* UIA_HIP_H */
