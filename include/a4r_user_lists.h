/* liba4r_hip.so: top-K recommendation and evaluation within a candidate list of each user's own.  Part of the C ABI of include/a4r.h, which includes
 * this file (new exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_user_lists.py, whose signature table
 * tests/test_user_lists_cpu.py holds against the prototypes below. */
#ifndef A4R_USER_LISTS_H
#define A4R_USER_LISTS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Every user brings a list of item ids -- the shortlist of a retrieval stage to re-rank, or the negatives drawn for a sampled evaluation -- as CSR:
 * list(u) = list_idx[list_ptr[u] .. list_ptr[u + 1]), list_ptr int32 [U + 1].  Only the first min(len, max_len) entries of a list are read (a negative
 * length counts as 0), never anything behind them; 0 <= max_len <= A4R_LIST_MAX, which the caller, who built the CSR, passes (it sizes the key
 * buffer in LDS).  Ids that are 0, negative or >= N1 are ignored and their table row is never dereferenced; an id listed more than once counts once.
 * excl / hist: CSR as a4r_topk_items' and a4r_eval_rank's, the first A4R_EVAL_MAX_HISTORY ids read, 0 and ids outside the table ignored.
 *   score(u, i) = <prec[u], item_emb[i]>, fp32, accumulated in a fixed order that depends on E alone (a lane's E / 16 products in sequence by fma,
 *            then a four-step butterfly over the row's 16 lanes): a pure function of (u, i), the same bits in every call, batch and list position.
 *            It is NOT promised to be the bits of the MFMA sweep of a4r_topk_items / a4r_eval_rank (the summation order differs); where every
 *            partial sum is exact in fp32 -- small-integer tables -- the two agree, which tests/test_user_lists_gpu.py holds them to.
 *   a4r_topk_lists: ids int32 [U, K] / scores fp32 [U, K] = the K best distinct items of list(u) that are not in excl(u), by score descending, ties by
 *            smaller id; fewer than K: the remaining slots are id 0 / -inf.  A NaN score ranks below -inf and is returned as the canonical quiet NaN;
 *            -0 is returned as +0 (the key rules of a4r_topk_items).
 *   a4r_eval_rank_lists: rank[u] = 1 + #{distinct i in list(u) : i not in hist(u), score(u, i) > score(u, target[u])}, the comparison strict and on the
 *            score alone (the ordered score halves of the keys; ids never enter), so a NaN score is below every number here as well.  The target
 *            need not be listed: its rank is the one it would have if it were.  A target that is no item (0, negative, >= N1) is never
 *            dereferenced and gets rank 1.
 * One launch, one 256-thread workgroup per user; no workspace, no atomics, nothing written but the outputs.  Any NULL pointer, U < 1, N1 < 2, E outside
 * {64, 128, 256, 512}, K outside 1 .. A4R_TOPK_MAX_K, max_len outside 0 .. A4R_LIST_MAX, or prec / item_emb not 16-byte aligned: A4R_EINVAL before
 * any HIP call. */
#define A4R_LIST_MAX 4096
int a4r_topk_lists(void* stream, const float* prec, const float* item_emb, const int32_t* list_ptr, const int32_t* list_idx,
                   const int32_t* excl_ptr, const int32_t* excl_idx, int32_t* ids, float* scores, int U, int N1, int E, int K, int max_len);
int a4r_eval_rank_lists(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* list_ptr,
                        const int32_t* list_idx, const int32_t* hist_ptr, const int32_t* hist_idx, int32_t* rank, int U, int N1, int E,
                        int max_len);

#ifdef __cplusplus
}
#endif
#endif
