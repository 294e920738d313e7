/* liba4r_hip.so: evaluation and top-K recommendation within a candidate set of items.  Part of the C ABI of include/a4r.h, which includes this file
 * (new exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_candidates.py, whose signature table
 * tests/test_candidates_cpu.py holds against the prototypes below. */
#ifndef A4R_CANDIDATES_H
#define A4R_CANDIDATES_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* A candidate set is one byte per row of the item table: cand uint8 [N1] on the device, item i is a candidate iff cand[i] != 0; cand[0] (the pad
 * row) is ignored.  One set is shared by all U users of a call.  Every other argument, the scores (the same fragments and MFMA chain, hence the
 * same bits), the shape, width and alignment rules and the refusals are those of the unmasked entry of include/a4r.h; a NULL cand returns
 * A4R_EINVAL before any launch, as any other NULL pointer does.
 *   a4r_eval_rank_cand:  rank[u] = 1 + #{i in 1..N1-1 : cand[i] != 0, i not in hist(u), score(u, i) > score(u, target[u])}.  The target need not be a
 *            candidate: its rank is then the one it would have if it were.  A history id that is no candidate changes nothing.
 *   a4r_topk_items_cand: the K best of the items 1..N1-1 with cand[i] != 0 that are not in excl(u); order, ties, pad slots (id 0 / -inf) of a short
 *            list, NaN and -0 rules, grid independence and the workspace (a4r_topk_ws_bytes(U, N1, K)) as documented for a4r_topk_items.
 * The set is read from global memory as it is (500 KB at 500 000 items: cache-resident); nothing is packed, copied to LDS or added with atomics. */
int a4r_eval_rank_cand(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* hist_ptr,
                       const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E);
int a4r_topk_items_cand(void* stream, const float* prec, const float* item_emb, const int32_t* excl_ptr, const int32_t* excl_idx,
                        const uint8_t* cand, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K);

#ifdef __cplusplus
}
#endif
#endif
