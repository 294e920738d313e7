/* liba4r_hip.so: evaluation and top-K recommendation with scores from the bf16 MFMA (--score_dtype bf16).  Part of the C ABI of include/a4r.h,
 * which includes this file (new exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_score_bf16.py, whose
 * signature table tests/test_score_bf16_cpu.py holds against the prototypes below. */
#ifndef A4R_SCORE_BF16_H
#define A4R_SCORE_BF16_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The rule.  prec_b = bf16(prec) [U, E] and table_b = bf16(item_emb) [N1, E], both rounded to nearest even on the bit pattern -- the copies
 * a4r_score_ce_bf16_cast writes (include/a4r_score_ce_bf16.h); there is no second cast.
 *   score(u, i) = <prec_b[u], table_b[i]>: products exact, accumulated in fp32 in one fixed chain -- E / 32 steps of v_mfma_f32_16x16x32_bf16, the
 *   32-element blocks of a row in ascending order, into a zeroed accumulator.  A score's bits depend on the two rows only: not on the tile or the
 *   column the item sits in, the row set the user sits in, the grid, or the entry.  a4r_eval_rank_bf16 and a4r_topk_items_bf16 hence give
 *   the same bits (tests/test_score_bf16_gpu.py holds them against each other).
 * Everything else is the contract of the fp32 entries of include/a4r.h and include/a4r_candidates.h, word for word:
 *   a4r_eval_rank_bf16:  rank[u] = 1 + #{i in 1..N1-1 : (cand == NULL or cand[i] != 0), i not in hist(u), score(u, i) > score(u, target[u])}; the
 *            target need not be a candidate; hist as CSR, at most A4R_EVAL_MAX_HISTORY ids of a user are read; ids 0, outside the table or
 *            repeated change nothing.  rank is overwritten (set to 1 by a launch of its own, then added to by integer atomics).
 *   a4r_topk_items_bf16: the K best of the items 1..N1-1 (with cand[i] != 0 when cand is given) that are not in excl(u) (at most
 *            A4R_EVAL_MAX_HISTORY ids of a user are read): score descending, ties by the smaller id; NaN orders below -inf, -0 equals +0; a user with fewer than K such items gets
 *            id 0 / score -inf in the remaining slots.  ws: a4r_topk_bf16_ws_bytes(U, N1, E, K) bytes, 8-byte aligned -- it follows the grid
 *            the bf16 kernels use, which hold 16 or 32 users a workgroup depending on E and K, so it is not a4r_topk_ws_bytes.
 *   Both: the same inputs give the same bits whatever the grid; no float atomics.
 * cand: uint8 [N1] on the device, one byte per table row, or NULL for all items.
 * E in {64, 128, 256, 512}, K in 1 .. A4R_TOPK_MAX_K, U >= 1, N1 >= 2, prec_b and table_b 16-byte aligned, ws 8-byte aligned, no required pointer
 * NULL; anything else returns A4R_EINVAL before any HIP call (a4r_topk_bf16_ws_bytes returns 0). */
size_t a4r_topk_bf16_ws_bytes(int U, int N1, int E, int K);
int a4r_eval_rank_bf16(void* stream, const void* prec_b, const void* table_b, const int32_t* target, const int32_t* hist_ptr,
                       const int32_t* hist_idx, const uint8_t* cand /* NULL: all items */, int32_t* rank, int U, int N1, int E);
int a4r_topk_items_bf16(void* stream, const void* prec_b, const void* table_b, const int32_t* excl_ptr, const int32_t* excl_idx,
                        const uint8_t* cand /* NULL: all items */, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K);

#ifdef __cplusplus
}
#endif
#endif
