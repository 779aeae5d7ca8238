// capi.cpp — extern "C" entry points of libuia_hip.so (declared in include/uia_hip.h).
// Thin: null checks on the descriptor, then the typed launcher.  No allocation, no sync.
#include "uia_kernels.h"

void uia_set_error(const char* fmt, ...);
#define NEED(ptr, name) do { if (!(ptr)) { uia_set_error("%s: null descriptor", name); return -1; } } while (0)

extern "C" {

int uia_version(void) { return 100; }

int uia_gemm(void* stream, int dtype, const uia_gemm_desc* d, int tile_cfg) {
    NEED(d, "uia_gemm");
    return uia_gemm_launch((hipStream_t)stream, dtype, *d, tile_cfg);
}
int uia_lora_rank_update(void* stream, int dtype, const uia_lora_rank_desc* d) {
    NEED(d, "uia_lora_rank_update");
    return uia_lora_rank_update_launch((hipStream_t)stream, dtype, *d);
}
int uia_ln_lora_down(void* stream, int dtype, const uia_ln_lora_desc* d) {
    NEED(d, "uia_ln_lora_down");
    return uia_ln_lora_down_launch((hipStream_t)stream, dtype, *d);
}
int uia_wgrad(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb, float alpha, float* dW, float* dbias_A) {
    return uia_wgrad_launch((hipStream_t)stream, dtype, M, I, J, A, lda, B, ldb, alpha, dW, dbias_A);
}
int uia_wgrad_ex(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb, float alpha, float* dW, int64_t ldw,
                 int i_valid, int j_valid, float* dbias_A) {
    if (ldw <= 0) { uia_set_error("uia_wgrad_ex: ldw=%lld must be positive", (long long)ldw); return -1; }
    return uia_wgrad_launch((hipStream_t)stream, dtype, M, I, J, A, lda, B, ldb, alpha, dW, dbias_A, ldw, i_valid, j_valid);
}
int uia_wgrad_group(void* stream, int dtype, const uia_wgrad_group_desc* d) {
    if (!d) { uia_set_error("uia_wgrad_group: null descriptor"); return -1; }
    if (d->n < 1 || d->n > 4) { uia_set_error("uia_wgrad_group: n=%d outside 1..4", d->n); return -1; }
    if (d->ldw <= 0) { uia_set_error("uia_wgrad_group: ldw=%lld must be positive", (long long)d->ldw); return -1; }
    float* dW[4];
    float* db[4];
    for (int g = 0; g < 4; ++g) { dW[g] = d->dW[g]; db[g] = d->dbias_A[g]; }
    if (d->drop_p > 0.f) for (int g = 0; g < d->n; ++g) if (db[g]) { uia_set_error("uia_wgrad_group: dbias with dropout on B is not a form of the kernel"); return -1; }
    return uia_wgrad_group_launch((hipStream_t)stream, dtype, d->n, d->M, d->I, d->J, d->A, (long)d->lda, d->B, (long)d->ldb, d->alpha, dW, db, (long)d->ldw, d->i_valid, d->j_valid,
                                  d->drop_p, d->drop_seed, (long)d->drop_ld, d->drop_col0);
}
int uia_wgrad_drop(void* stream, int dtype, int M, int I, int J, const void* A, int64_t lda, const void* B, int64_t ldb, float alpha, float* dW, int64_t ldw,
                   int i_valid, int j_valid, float drop_p, uint64_t seed, int64_t drop_ld, int drop_col0) {
    if (ldw <= 0) { uia_set_error("uia_wgrad_drop: ldw=%lld must be positive", (long long)ldw); return -1; }
    if (!(drop_p > 0.f)) { uia_set_error("uia_wgrad_drop: drop_p=%f must be in (0, 1); uia_wgrad_ex is the form without dropout", (double)drop_p); return -1; }
    return uia_wgrad_launch((hipStream_t)stream, dtype, M, I, J, A, lda, B, ldb, alpha, dW, nullptr, ldw, i_valid, j_valid, drop_p, seed, drop_ld, drop_col0);
}
int uia_attn_fwd(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_fwd");
    return uia_attn_fwd_launch((hipStream_t)stream, dtype, *d);
}
int uia_attn_fwd_long(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_fwd_long");
    return uia_attn_fwd_long_launch((hipStream_t)stream, dtype, *d);
}
int uia_attn_bwd(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_bwd");
    return uia_attn_bwd_launch((hipStream_t)stream, dtype, *d, 0);
}
int uia_attn_bwd_cfg(void* stream, int dtype, const uia_attn_desc* d, int cfg) {
    NEED(d, "uia_attn_bwd_cfg");
    return uia_attn_bwd_launch((hipStream_t)stream, dtype, *d, cfg);
}
int uia_layernorm_fwd(void* stream, int dtype, int M, int D, int64_t ldx, const float* x, const float* gamma, const float* beta, float eps, void* yT, float* y32) {
    return uia_layernorm_fwd_launch((hipStream_t)stream, dtype, M, D, ldx, x, gamma, beta, eps, yT, y32, nullptr);
}
int uia_layernorm_fwd_stats(void* stream, int dtype, int M, int D, int64_t ldx, const float* x, const float* gamma, const float* beta, float eps, void* yT, float* y32,
                            float* stats) {
    return uia_layernorm_fwd_launch((hipStream_t)stream, dtype, M, D, ldx, x, gamma, beta, eps, yT, y32, stats);
}
int uia_layernorm_bwd(void* stream, int dtype, int M, int D, int64_t ldx, const void* dy, const float* x, const float* gamma, float eps, const float* dres, float* dx32, void* dxT) {
    return uia_layernorm_bwd_launch((hipStream_t)stream, dtype, M, D, ldx, dy, x, gamma, eps, dres, dx32, dxT);
}
int uia_layernorm_bwd3(void* stream, int dtype, int M, int D, int64_t ldx, const void* dy, const float* x, const void* x_hi, const int8_t* x_lo, int64_t x_kb_rows,
                       const float* gamma, float eps, const float* dres, const void* dres_hi, const int8_t* dres_lo, int64_t dres_kb_rows, float* dx32, void* dxT,
                       int8_t* dx_lo) {
    return uia_layernorm_bwd3_launch((hipStream_t)stream, dtype, M, D, ldx, dy, x, x_hi, x_lo, (long)x_kb_rows, gamma, eps, dres, dres_hi, dres_lo, (long)dres_kb_rows, dx32, dxT,
                                     dx_lo);
}
int uia_layernorm_bwd_periodic(void* stream, int dtype, int M, int D, const void* dy, const float* x, const void* x_hi, const int8_t* x_lo, int64_t x_kb_rows,
                               const float* gamma, float eps, const float* dres_rows, int period, float* dx32, void* dxT, int8_t* dx_lo) {
    return uia_layernorm_bwd_periodic_launch((hipStream_t)stream, dtype, M, D, dy, x, x_hi, x_lo, (long)x_kb_rows, gamma, eps, dres_rows, period, dx32, dxT, dx_lo);
}
int uia_attn_bwd_cls(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_bwd_cls");
    return uia_attn_bwd_cls_launch((hipStream_t)stream, dtype, *d);
}
int uia_attn_bwd_cls_rows(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_bwd_cls_rows");
    return uia_attn_bwd_cls_launch((hipStream_t)stream, dtype, *d, true);
}
int uia_attn_fwd_cls(void* stream, int dtype, const uia_attn_desc* d) {
    NEED(d, "uia_attn_fwd_cls");
    return uia_attn_fwd_cls_launch((hipStream_t)stream, dtype, *d);
}
int uia_mona_cls_fwd(void* stream, int dtype, int B, int ntok, const void* t, int64_t ldt, void* d, float p_drop, uint64_t seed, const uint8_t* keep_mask) {
    return uia_mona_cls_fwd_launch((hipStream_t)stream, dtype, B, ntok, t, (long)ldt, d, p_drop, seed, keep_mask);
}
int uia_rows3_to_f32(void* stream, int rows, int D, int64_t stride_rows, const void* hi, int64_t ldhi, int64_t hi_kb_rows, const int8_t* lo, int64_t ldlo, float* dst) {
    return uia_rows3_to_f32_launch((hipStream_t)stream, rows, D, (long)stride_rows, hi, (long)ldhi, (long)hi_kb_rows, lo, (long)ldlo, dst);
}
int uia_mona_cls_bwd(void* stream, int dtype, int B, int ntok, const void* dd, const void* t, int64_t ldt, void* dt, float p_drop, uint64_t seed, const uint8_t* keep_mask) {
    return uia_mona_cls_bwd_launch((hipStream_t)stream, dtype, B, ntok, dd, t, (long)ldt, dt, p_drop, seed, keep_mask);
}
int uia_copy_rows(void* stream, int rows, int64_t row_bytes, const void* src, int64_t src_stride_bytes, void* dst) {
    return uia_copy_rows_launch((hipStream_t)stream, rows, (long)row_bytes, src, (long)src_stride_bytes, dst);
}
int uia_cast(void* stream, int dtype, size_t n, const float* src, void* dst, float scale) { return uia_cast_launch((hipStream_t)stream, dtype, n, src, dst, scale); }
int uia_transpose_cast(void* stream, int dtype, int rows, int cols, const float* src, void* dst) { return uia_transpose_cast_launch((hipStream_t)stream, dtype, rows, cols, src, dst); }
int uia_pack_weights(void* stream, int dtype, int n, const uia_pack_desc* descs_device, int max_elems) { return uia_pack_weights_launch((hipStream_t)stream, dtype, n, descs_device, max_elems); }
int uia_im2col(void* stream, int dtype, int B, int C, int H, int W, int P, const float* img, void* out) { return uia_im2col_launch((hipStream_t)stream, dtype, B, C, H, W, P, img, out); }
int uia_fill_cls(void* stream, int B, int N, int D, const float* cls, const float* pos0, float* x) { return uia_fill_cls_launch((hipStream_t)stream, B, N, D, cls, pos0, x); }
int uia_embed(void* stream, int rows, int L, int D, int vocab, int max_pos, const int64_t* ids, const float* table, const float* pos, const float* type0, float* out) {
    return uia_embed_launch((hipStream_t)stream, rows, L, D, vocab, max_pos, ids, table, pos, type0, out);
}
int uia_gather_rows(void* stream, int n, int D, const float* src, const int64_t* idx, float* dst) { return uia_gather_rows_launch((hipStream_t)stream, n, D, src, idx, dst); }

int uia_mona_pre_fwd(void* stream, int dtype, int M, int D, const float* x, const float* norm_w, const float* norm_b, const float* gamma,
                     const float* gammax, float eps, void* u) {
    return uia_mona_pre_fwd_launch((hipStream_t)stream, dtype, M, D, x, norm_w, norm_b, gamma, gammax, eps, u);
}
int uia_mona_pre_bwd(void* stream, int dtype, int M, int D, const void* du, const float* x, const float* dy, const float* norm_w,
                     const float* norm_b, const float* gamma, const float* gammax, float eps, float* dx32, void* dxT, float* g_gamma,
                     float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws, int64_t dxT_kb_rows) {
    return uia_mona_pre_bwd_launch((hipStream_t)stream, dtype, M, D, du, x, dy, norm_w, norm_b, gamma, gammax, eps, dx32, dxT, g_gamma, g_gammax,
                                   g_norm_w, g_norm_b, ws, (long)dxT_kb_rows);
}
int uia_mona_pre_fwd_t(void* stream, int dtype, int M, int D, const float* x, const float* norm_w, const float* norm_b, const float* gamma, const float* gammax,
                       float eps, void* u, const void* w1, int64_t ldw1, const float* b1, void* t, int64_t ldt) {
    return uia_mona_pre_fwd_t_launch((hipStream_t)stream, dtype, M, D, x, norm_w, norm_b, gamma, gammax, eps, u, w1, (long)ldw1, b1, t, (long)ldt);
}
int uia_mona_pre_bwd_du(void* stream, int dtype, int M, int D, const void* dt, int64_t ldt, const void* w1t, int64_t ldw1, const float* x, const float* dy,
                        const float* norm_w, const float* norm_b, const float* gamma, const float* gammax, float eps, float* dx32, void* dxT, float* g_gamma,
                        float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws, int64_t dxT_kb_rows) {
    if (!dt || !w1t) { uia_set_error("uia_mona_pre_bwd_du: null dt / w1t"); return -1; }
    return uia_mona_pre_bwd_launch((hipStream_t)stream, dtype, M, D, nullptr, x, dy, norm_w, norm_b, gamma, gammax, eps, dx32, dxT, g_gamma, g_gammax,
                                   g_norm_w, g_norm_b, ws, (long)dxT_kb_rows, dt, (long)ldt, w1t, (long)ldw1);
}
int uia_mona_pre_bwd_du3(void* stream, int dtype, int M, int D, const void* dt, int64_t ldt, const void* w1t, int64_t ldw1, const float* x, const void* dy_hi, const int8_t* dy_lo,
                         const float* norm_w, const float* norm_b, const float* gamma, const float* gammax, float eps, void* dxT, int8_t* dx_lo, float* g_gamma,
                         float* g_gammax, float* g_norm_w, float* g_norm_b, float* ws, int64_t dxT_kb_rows) {
    if (!dt || !w1t || !dy_hi || !dy_lo || !dx_lo) { uia_set_error("uia_mona_pre_bwd_du3: null dt / w1t / dy_hi / dy_lo / dx_lo"); return -1; }
    return uia_mona_pre_bwd_launch((hipStream_t)stream, dtype, M, D, nullptr, x, nullptr, norm_w, norm_b, gamma, gammax, eps, nullptr, dxT, g_gamma, g_gammax,
                                   g_norm_w, g_norm_b, ws, (long)dxT_kb_rows, dt, (long)ldt, w1t, (long)ldw1, dy_hi, dy_lo, dx_lo);
}
size_t uia_mona_pre_bwd_workspace_bytes(int M, int D) { return uia_mona_pre_bwd_ws_floats(M, D) * sizeof(float); }
int uia_mona_spatial_fwd(void* stream, int dtype, const uia_mona_spatial_desc* d) {
    NEED(d, "uia_mona_spatial_fwd");
    return uia_mona_spatial_fwd_launch((hipStream_t)stream, dtype, *d);
}
int uia_mona_spatial_bwd(void* stream, int dtype, const uia_mona_spatial_desc* d) {
    NEED(d, "uia_mona_spatial_bwd");
    return uia_mona_spatial_bwd_launch((hipStream_t)stream, dtype, *d);
}
int uia_mona_fused_fwd(void* stream, int dtype, const uia_mona_fused_desc* d) {
    NEED(d, "uia_mona_fused_fwd");
    return uia_mona_fused_fwd_launch((hipStream_t)stream, dtype, *d);
}

size_t uia_infonce_workspace_bytes(int B, int E) { return uia_infonce_workspace_floats(B, E) * sizeof(float); }
int uia_infonce_fwd_bwd(void* stream, int B, int E, const float* img, const float* txt, float inv_temp, float grad_scale, float* loss,
                        float* dimg, float* dtxt, void* workspace, size_t workspace_bytes) {
    return uia_infonce_launch((hipStream_t)stream, B, E, img, txt, inv_temp, grad_scale, loss, dimg, dtxt, (float*)workspace, workspace_bytes / sizeof(float));
}
int uia_adamw_clip_step(void* stream, size_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float max_norm, int step, float grad_scale, float* ws2) {
    return uia_adamw_clip_launch((hipStream_t)stream, n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, max_norm, step, grad_scale, ws2);
}
int uia_grad_accum_guarded(void* stream, size_t n, float* acc, float* mb, const float* loss, float* stats, int32_t* ctl, uint8_t* ok_log, int64_t log_index) {
    return uia_grad_accum_guarded_launch((hipStream_t)stream, n, acc, mb, loss, stats, (int*)ctl, ok_log, (long)log_index);
}
int uia_adamw_clip_step_guarded(void* stream, size_t n, float* p, float* acc, float* m, float* v, float lr, float lr_min, int t_max, float beta1, float beta2,
                                float eps, float weight_decay, float max_norm, float grad_scale, float skip_scale, float* ws8, int32_t* ctl) {
    return uia_adamw_clip_guarded_launch((hipStream_t)stream, n, p, acc, m, v, lr, lr_min, t_max, beta1, beta2, eps, weight_decay, max_norm, grad_scale, skip_scale, ws8, (int*)ctl);
}

int uia_dropout(void* stream, int dtype, size_t n, const void* src, void* dst, float p, uint64_t seed, int accumulate) {
    return uia_dropout_launch((hipStream_t)stream, dtype, n, src, dst, p, seed, accumulate);
}
int uia_colsum(void* stream, int dtype, int M, int N, const void* A, int64_t lda, float* out) {
    return uia_colsum_launch((hipStream_t)stream, dtype, M, N, A, lda, out);
}

int uia_layernorm_bwd_affine(void* stream, int dtype, int M, int D, const void* dy, const float* x, const float* gamma, float eps, const float* dres,
                             float* dx32, float* g_gamma, float* g_beta) {
    return uia_layernorm_bwd_affine_launch((hipStream_t)stream, dtype, M, D, dy, x, gamma, eps, dres, dx32, g_gamma, g_beta);
}
int uia_film_fwd(void* stream, int B, int N, int C, const float* x, const float* mul, const float* add, float* y) { return uia_film_fwd_launch((hipStream_t)stream, B, N, C, x, mul, add, y); }
int uia_film_bwd(void* stream, int B, int N, int C, const float* dy, const float* x, const float* mul, float* dx, float* dmul, float* dadd) {
    return uia_film_bwd_launch((hipStream_t)stream, B, N, C, dy, x, mul, dx, dmul, dadd);
}
int uia_im2col3x3(void* stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const float* x, void* cols) {
    return uia_im2col3x3_launch((hipStream_t)stream, dtype, B, h, w, C, ntok, tok_off, x, cols);
}
int uia_col2im3x3(void* stream, int dtype, int B, int h, int w, int C, int ntok, int tok_off, const void* dcols, float* dx) {
    return uia_col2im3x3_launch((hipStream_t)stream, dtype, B, h, w, C, ntok, tok_off, dcols, dx);
}
int uia_unshuffle(void* stream, int dtype, int B, int h, int w, int k1, int k2, const void* tmp, int64_t ld, float bias, float* out) {
    return uia_unshuffle_launch((hipStream_t)stream, dtype, B, h, w, k1, k2, tmp, ld, bias, out);
}
int uia_shuffle(void* stream, int dtype, int B, int h, int w, int k1, int k2, const float* dout, void* dtmp, int64_t ld) {
    return uia_shuffle_launch((hipStream_t)stream, dtype, B, h, w, k1, k2, dout, dtmp, ld);
}
int uia_act_bwd(void* stream, int dtype, size_t n, const void* dy, const void* y, int act, void* out) { return uia_act_bwd_launch((hipStream_t)stream, dtype, n, dy, y, act, out); }

size_t uia_mona_spatial_workspace_bytes(int B) { return uia_mona_spatial_ws_floats(B) * sizeof(float); }

int uia_upsample_bilinear_fwd(void* stream, int B, int C, int h, int w, int H, int W, const float* src, int64_t ld, float* dst) {
    return uia_upsample_bilinear_launch((hipStream_t)stream, false, B, C, h, w, H, W, src, dst, (long)ld);
}
int uia_upsample_bilinear_bwd(void* stream, int B, int C, int h, int w, int H, int W, const float* ddst, float* dsrc, int64_t ld) {
    return uia_upsample_bilinear_launch((hipStream_t)stream, true, B, C, h, w, H, W, ddst, dsrc, (long)ld);
}
int uia_segment_mean_fwd(void* stream, int B, int n, int C, const float* x, int64_t ld, float* out) {
    return uia_segment_mean_launch((hipStream_t)stream, false, B, n, C, x, out, (long)ld);
}
int uia_segment_mean_bwd(void* stream, int B, int n, int C, const float* dout, float* dx, int64_t ld) {
    return uia_segment_mean_launch((hipStream_t)stream, true, B, n, C, dout, dx, (long)ld);
}

size_t uia_dicece_workspace_bytes(int B) { return uia_dicece_ws_floats(B) * sizeof(float); }
int uia_dicece_fwd_bwd(void* stream, int B, int C, int HW, const float* logits, const float* label, float smooth_nr, float smooth_dr,
                       float* ws, float* loss, float* dlogits) {
    return uia_dicece_launch((hipStream_t)stream, B, C, HW, logits, label, smooth_nr, smooth_dr, ws, loss, dlogits);
}

size_t uia_focal_workspace_bytes(int N, int C) { return uia_focal_ws_bytes(N, C); }
int uia_focal_fwd_bwd(void* stream, int N, int C, const float* logits, const int64_t* labels, float gamma, float alpha, void* ws, size_t ws_bytes,
                      float* loss, float* dlogits) {
    return uia_focal_launch((hipStream_t)stream, N, C, logits, labels, gamma, alpha, ws, ws_bytes, loss, dlogits);
}
size_t uia_binary_cls_stats_workspace_bytes(int N) { return uia_binary_cls_stats_ws_bytes(N); }
int uia_binary_cls_stats(void* stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes, double* record) {
    return uia_binary_cls_stats_launch((hipStream_t)stream, N, p1, labels, perm, ws, ws_bytes, record);
}

size_t uia_surface_distances_workspace_bytes(int B, int H, int W) { return uia_surface_ws_bytes(B, H, W); }
int uia_surface_distances(void* stream, int B, int H, int W, const float* logits, const float* label, float percentile, void* ws, size_t ws_bytes,
                          double* hd, double* asd) {
    return uia_surface_launch((hipStream_t)stream, B, H, W, logits, label, percentile, ws, ws_bytes, hd, asd);
}

int uia_seg_viz(void* stream, int B, int C, int Ci, int S, const float* logits, const float* images, const void* labels, int label_dtype,
                uint8_t* mask_rgb, uint8_t* overlay_rgb, uint8_t* pred) {
    return uia_seg_viz_launch((hipStream_t)stream, B, C, Ci, S, logits, images, labels, label_dtype, mask_rgb, overlay_rgb, pred);
}

size_t uia_retrieval_workspace_bytes(int N, int E) { return uia_retrieval_ranks_ws_bytes(N, E); }
int uia_retrieval_ranks(void* stream, int N, int E, const float* img, const float* txt, int normalize, void* ws, size_t ws_bytes,
                        int32_t* gt_i2t, int32_t* eq_i2t, int32_t* gt_t2i, int32_t* eq_t2i) {
    return uia_retrieval_ranks_launch((hipStream_t)stream, N, E, img, txt, normalize, ws, ws_bytes, gt_i2t, eq_i2t, gt_t2i, eq_t2i);
}
size_t uia_retrieval_stats_workspace_bytes(int N) { return uia_retrieval_stats_ws_bytes(N); }
int uia_retrieval_stats(void* stream, int N, const int32_t* gt, int nk, const int32_t* k_values, void* ws, size_t ws_bytes, double* record) {
    return uia_retrieval_stats_launch((hipStream_t)stream, N, gt, nk, k_values, ws, ws_bytes, record);
}
size_t uia_retrieval_topk_workspace_bytes(int Q, int N, int E, int K) { return uia_retrieval_topk_ws_bytes(Q, N, E, K); }
int uia_retrieval_topk_splits(int Q, int N) { return uia_retrieval_topk_rule(Q, N); }
int uia_retrieval_topk(void* stream, int Q, int N, int E, int K, const float* queries, const float* gallery, int normalize, int splits, void* ws,
                       size_t ws_bytes, int32_t* idx, float* score) {
    return uia_retrieval_topk_launch((hipStream_t)stream, Q, N, E, K, queries, gallery, normalize, splits, ws, ws_bytes, idx, score);
}

int uia_zero_shot_score(void* stream, int N, int T, int E, int C, const int32_t* class_off, const float* img, const float* prompts, float* logits, int64_t ld,
                        int64_t row, float* probs, float* img_n) {
    return uia_zero_shot_score_launch((hipStream_t)stream, N, T, E, C, class_off, img, prompts, logits, (long)ld, (long)row, probs, img_n);
}
size_t uia_binary_roc_curve_workspace_bytes(int N) { return uia_binary_roc_curve_ws_bytes(N); }
int uia_binary_roc_curve(void* stream, int N, const float* p1, const int64_t* labels, const int64_t* perm, void* ws, size_t ws_bytes, int32_t* count,
                         double* fpr, double* tpr, float* thr) {
    return uia_binary_roc_curve_launch((hipStream_t)stream, N, p1, labels, perm, ws, ws_bytes, count, fpr, tpr, thr);
}

size_t uia_augment_workspace_bytes(int B, int S) { return uia_augment_ws_bytes(B, S); }
int uia_augment_batch(void* stream, int B, int S, const float* images, const uint8_t* masks, const int32_t* programs, void* ws, size_t ws_bytes,
                      float* out_images, uint8_t* out_masks) {
    return uia_augment_batch_launch((hipStream_t)stream, B, S, images, masks, programs, ws, ws_bytes, out_images, out_masks);
}
int uia_augment_gather(void* stream, int N, int B, int S, int src_dtype, const void* images, const uint8_t* masks, const int32_t* programs, void* ws,
                       size_t ws_bytes, float* out_images, uint8_t* out_masks) {
    return uia_augment_gather_launch((hipStream_t)stream, N, B, S, src_dtype, images, masks, programs, ws, ws_bytes, out_images, out_masks);
}

size_t uia_resize_workspace_bytes(int B) { return uia_resize_ws_bytes(B); }
int uia_resize_batch(void* stream, int B, int C, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes, float* out_images,
                     uint8_t* out_masks) {
    return uia_resize_batch_launch((hipStream_t)stream, B, C, S, src, src_bytes, desc, ws, ws_bytes, out_images, out_masks);
}
int uia_resize_batch_rgb(void* stream, int B, int S, const uint8_t* src, size_t src_bytes, const int32_t* desc, void* ws, size_t ws_bytes, float* out_images) {
    return uia_resize_batch_rgb_launch((hipStream_t)stream, B, S, src, src_bytes, desc, ws, ws_bytes, out_images);
}

size_t uia_seg_native_workspace_bytes(int B) { return uia_seg_native_ws_bytes(B); }
int uia_seg_predict_native(void* stream, int B, int S, const float* logits, const uint8_t* src, size_t src_bytes, const int32_t* desc, uint8_t* out,
                           size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats) {
    return uia_seg_predict_native_launch((hipStream_t)stream, B, S, logits, src, src_bytes, desc, out, out_bytes, ws, ws_bytes, stats);
}

size_t uia_seg_native_ens_workspace_bytes(int B) { return uia_seg_native_ens_ws_bytes(B); }
int uia_seg_predict_native_ens(void* stream, int K, int B, int S, const float* logits, uint32_t flips, float threshold, const uint8_t* src, size_t src_bytes,
                               const int32_t* desc, uint8_t* out, size_t out_bytes, void* ws, size_t ws_bytes, int32_t* stats, uint64_t* sums) {
    return uia_seg_predict_native_ens_launch((hipStream_t)stream, K, B, S, logits, flips, threshold, src, src_bytes, desc, out, out_bytes, ws, ws_bytes, stats, sums);
}

size_t uia_mask_components_workspace_bytes(int B, int64_t pixels) { return uia_mask_components_ws_bytes(B, pixels); }
int uia_mask_components(void* stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats, int32_t* list, int max_list) {
    return uia_mask_components_launch((hipStream_t)stream, B, buf, buf_bytes, desc, ws, ws_bytes, stats, list, max_list);
}

size_t uia_mask_morphology_workspace_bytes(int B, int64_t pixels) { return uia_mask_morphology_ws_bytes(B, pixels); }
int uia_mask_morphology(void* stream, int B, uint8_t* buf, size_t buf_bytes, const int32_t* desc, void* ws, size_t ws_bytes, int32_t* stats) {
    return uia_mask_morphology_launch((hipStream_t)stream, B, buf, buf_bytes, desc, ws, ws_bytes, stats);
}

int uia_im2col_padded(void* stream, int dtype, int B, int C, int H, int W, int P, const float* img, void* cols, int64_t ldo) {
    return uia_im2col_padded_launch((hipStream_t)stream, dtype, B, C, H, W, P, img, cols, (long)ldo);
}

int uia_embed_bwd(void* stream, int rows, int D, int vocab, const int64_t* ids, const float* dx, float* dtable, int64_t pad_id) {
    return uia_embed_bwd_launch((hipStream_t)stream, rows, D, vocab, ids, dx, dtable, (long)pad_id);
}

int uia_embed_packed(void* stream, int rows, int D, int vocab, int max_pos, const int64_t* ids, const int64_t* pos_idx, const float* table,
                     const float* pos, const float* type0, float* out) {
    return uia_embed_packed_launch((hipStream_t)stream, rows, D, vocab, max_pos, ids, pos_idx, table, pos, type0, out);
}

}  // extern "C"
int uia_ln_mean_rows(void* stream, int B, int L, int row0, int n, int D, int64_t ldx, const float* x, const float* gamma, const float* beta,
                     float eps, float* ws, float* out, int64_t ldo) {
    return uia_ln_mean_rows_launch((hipStream_t)stream, B, L, row0, n, D, (long)ldx, x, gamma, beta, eps, ws, out, (long)ldo);
}

extern "C" {
int uia_conv_igemm(void* stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N, int N1,
                   const void* w, const float* bias, void* y1, void* y2) {
    return uia_conv_igemm_launch((hipStream_t)stream, dtype, mode, B, H, W, C1, C2, x1, x2, N, N1, w, bias, y1, y2);
}
int uia_conv_wgrad(void* stream, int dtype, int mode, int B, int H, int W, int C1, int C2, const void* x1, const void* x2, int N, const void* dy,
                   float* ws, float* dw) {
    return uia_conv_wgrad_launch((hipStream_t)stream, dtype, mode, B, H, W, C1, C2, x1, x2, N, dy, ws, dw);
}
int uia_bn_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const float* gamma, const float* beta, float* running_mean,
               float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean, float* invstd, float* scale,
               float* shift, int relu, void* out) {
    return uia_bn_fwd_launch((hipStream_t)stream, dtype, training, (long)M, C, y, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps,
                             ws, mean, invstd, scale, shift, relu, out);
}
int uia_bn_relu_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                    const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy) {
    return uia_bn_relu_bwd_launch((hipStream_t)stream, dtype, (long)M, C, y, dout, scale, shift, mean, invstd, gamma, ws, dgamma, dbeta, dy);
}
int uia_colsum_ordered(void* stream, int dtype, int64_t M, int C, const void* y, float* ws, float* out) {
    return uia_colsum_ordered_launch((hipStream_t)stream, dtype, (long)M, C, y, ws, out);
}
int uia_bn_act_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean, float* invstd, float* scale,
                   float* shift, float slope, void* out, float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    return uia_bn_act_fwd_launch((hipStream_t)stream, dtype, training, (long)M, C, y, gamma, beta, running_mean, running_var, num_batches_tracked, momentum,
                                 eps, ws, mean, invstd, scale, shift, slope, out, drop_p, seed, keep_mask);
}
int uia_bn_act_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* dout, const float* scale, const float* shift,
                   const float* mean, const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, float slope,
                   float drop_p, uint64_t seed, const uint8_t* keep_mask) {
    return uia_bn_act_bwd_launch((hipStream_t)stream, dtype, (long)M, C, y, dout, scale, shift, mean, invstd, gamma, ws, dgamma, dbeta, dy, slope, drop_p,
                                 seed, keep_mask);
}
int uia_maxpool2_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, void* y) {
    return uia_maxpool2_launch((hipStream_t)stream, dtype, 0, B, H, W, C, x, nullptr, y);
}
int uia_maxpool2_bwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, const void* dy, void* dx) {
    return uia_maxpool2_launch((hipStream_t)stream, dtype, 1, B, H, W, C, x, dy, dx);
}
int uia_conv_strided(void* stream, int dtype, int dgrad, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* w, void* y) {
    return uia_conv_strided_launch((hipStream_t)stream, dtype, dgrad, B, H, W, C, k, s, x, N, w, y);
}
int uia_conv_strided_wgrad(void* stream, int dtype, int B, int H, int W, int C, int k, int s, const void* x, int N, const void* dy, float* ws,
                           float* dw) {
    return uia_conv_strided_wgrad_launch((hipStream_t)stream, dtype, B, H, W, C, k, s, x, N, dy, ws, dw);
}
int uia_maxpool3s2_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, void* y) {
    return uia_maxpool3s2_launch((hipStream_t)stream, dtype, 0, B, H, W, C, x, nullptr, y);
}
int uia_maxpool3s2_bwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, const void* dy, void* dx) {
    return uia_maxpool3s2_launch((hipStream_t)stream, dtype, 1, B, H, W, C, x, dy, dx);
}
int uia_bn_add_relu_fwd(void* stream, int dtype, int training, int64_t M, int C, const void* y, const void* r, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum, float eps, float* ws, float* mean,
                        float* invstd, float* scale, float* shift, void* out) {
    return uia_bn_add_relu_fwd_launch((hipStream_t)stream, dtype, training, (long)M, C, y, r, gamma, beta, running_mean, running_var, num_batches_tracked,
                                      momentum, eps, ws, mean, invstd, scale, shift, out);
}
int uia_bn_add_relu_bwd(void* stream, int dtype, int64_t M, int C, const void* y, const void* out, const void* dout, const float* mean,
                        const float* invstd, const float* gamma, float* ws, float* dgamma, float* dbeta, void* dy, void* dr) {
    return uia_bn_add_relu_bwd_launch((hipStream_t)stream, dtype, (long)M, C, y, out, dout, mean, invstd, gamma, ws, dgamma, dbeta, dy, dr);
}
int uia_avgpool_fwd(void* stream, int dtype, int B, int H, int W, int C, const void* x, float* pooled) {
    return uia_avgpool_launch((hipStream_t)stream, dtype, 0, B, H, W, C, x, pooled, nullptr);
}
int uia_avgpool_bwd(void* stream, int dtype, int B, int H, int W, int C, const float* dout, void* dx) {
    return uia_avgpool_launch((hipStream_t)stream, dtype, 1, B, H, W, C, nullptr, const_cast<float*>(dout), dx);
}
int uia_nchw_to_nhwc(void* stream, int dtype, int B, int Cin, int H, int W, int Cout, int rep, const float* x, void* out) {
    return uia_nchw_to_nhwc_launch((hipStream_t)stream, dtype, B, Cin, H, W, Cout, rep, x, out);
}
int uia_add2(void* stream, int dtype, int64_t n, const void* a, const void* b, void* out) {
    return uia_add2_launch((hipStream_t)stream, dtype, (long)n, a, b, out);
}
int uia_upsample_ac(void* stream, int dtype, int backward, int B, int H, int W, int C, int f, const void* in, void* out) {
    return uia_upsample_ac_launch((hipStream_t)stream, dtype, backward, B, H, W, C, f, in, out);
}
int uia_resize_aa(void* stream, int dtype, int backward, int B, int C, int Hi, int Wi, int Ho, int Wo, const void* x, float* tmp, float* out,
                  const float* dout, void* dx) {
    return uia_resize_aa_launch((hipStream_t)stream, dtype, backward, B, C, Hi, Wi, Ho, Wo, x, tmp, out, dout, dx);
}
}  // extern "C"
