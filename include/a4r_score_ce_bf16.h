/* liba4r_hip.so: the full-softmax cross-entropy head of the ID tower on the bf16 MFMA (--ce_dtype bf16).  Part of the C ABI of include/a4r.h, which
 * includes this file (new exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_ce_bf16.py, whose signature
 * table tests/test_score_ce_bf16_cpu.py holds against the prototypes below. */
#ifndef A4R_SCORE_CE_BF16_H
#define A4R_SCORE_CE_BF16_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The head of a4r_score_ce_* (include/a4r.h) evaluated
 * at prec_b = bf16(prec) [R, E] and table_b = bf16(table) [N1, E], both rounded to nearest even: scores <prec_b[r], table_b[i]> accumulated in fp32,
 * lse, s_tgt, loss_ws, trained(r), count and g as stated there.  The gradients are those with respect to prec_b and table_b, meant to be handed unchanged to
 * the fp32 masters (straight-through): d_prec = g / count x (sum_i p[r, i] table_b[i] - table_b[tgt[r]]), d_table[i, :] += g / count x sum over
 * trained r of (p[r, i] - [i == tgt[r]]) prec_b[r].  One further rounding: the probability tile (bwd_rows) and the coefficient tile p - [i == tgt]
 * (bwd_items) are rounded to bf16 as the A operand of the second product, which accumulates in fp32.  Everything else is the fp32 head's contract:
 * exact zeros in d_prec on rows not trained, row 0 of d_table never written, count == 0 or g == 0 writes nothing into d_table, no float atomics, a
 * fixed summation order, ws = a4r_score_ce_bf16_ws_bytes(R, N1, E, ranges) bytes (ranges x R x E floats, independent of N1), 16-byte aligned.
 *   a4r_score_ce_bf16_cast: dst[k] = bf16(src[k]), k < n (RNE on the bit pattern, denormals kept, NaN stays NaN); src and dst 16-byte aligned, n >= 1.
 *   A workgroup holds A4R_SCORE_CE_BF16_ROWS rows; ranges 0 = a4r_score_ce_bf16_ranges(R, N1), chosen from the CU count over groups of that many rows.
 * E in {64, 128}, R >= 1, N1 >= 2, ranges in 0 .. 32, prec_b and table_b 16-byte aligned; anything else returns A4R_EINVAL before any launch
 * (a4r_score_ce_bf16_ws_bytes returns 0). */
#define A4R_SCORE_CE_BF16_ROWS 64
int a4r_score_ce_bf16_cast(void* stream, const float* src, void* dst, int64_t n);
size_t a4r_score_ce_bf16_ws_bytes(int R, int N1, int E, int ranges);
int a4r_score_ce_bf16_ranges(int R, int N1);
int a4r_score_ce_bf16_fwd(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask, float* lse,
                          float* s_tgt, float* loss_ws, void* ws, int R, int N1, int E, int ranges);
int a4r_score_ce_bf16_bwd_rows(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                               const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_prec,
                               void* ws, int R, int N1, int E, int ranges);
int a4r_score_ce_bf16_bwd_items(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                                const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table,
                                int ldg, int R, int N1, int E);

#ifdef __cplusplus
}
#endif
#endif
