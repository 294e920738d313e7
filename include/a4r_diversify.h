/* liba4r_hip.so: diversified re-ranking of a top-K list (maximal marginal relevance).  Part of the C ABI of include/a4r.h, which includes this file
 * (a new export, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_diversify.py, whose signature table
 * tests/test_mmr_cpu.py holds against the prototype below. */
#ifndef A4R_DIVERSIFY_H
#define A4R_DIVERSIFY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Every user brings a pool of P entries (pool_ids[u, j], pool_scores[u, j]), j = 0 .. P-1 -- in practice the sorted output of a4r_topk_items,
 * a4r_topk_items_cand or a4r_topk_lists with K = P, but the rule is positional and assumes no order.  Stated in real arithmetic:
 *   valid      entry j is valid iff 1 <= pool_ids[j] < N1 and pool_scores[j] is finite.  Pads (id 0 / -inf), ids outside the table and NaN / inf scores
 *              are invalid: never selected, and their table row is never dereferenced.
 *   relevance  r[j] = (ps[j] - smin) / (smax - smin), smin / smax over the valid entries; r[j] = 1 for every valid j when smax == smin.
 *   similarity c(i, j) = <e_i, e_j> / (sqrt(<e_i, e_i>) * sqrt(<e_j, e_j>)), e_j = item_emb[pool_ids[j]]; c = 0 when either norm is 0.  Two entries with
 *              the same id are two entries, with c = 1.
 *   selection  for t = 0 .. K-1, among the valid unselected j: v[j] = lambda * r[j] - (1 - lambda) * m[j], m[j] = the largest c(i, j) over the
 *              selected i (0 while nothing is selected); the j with the largest v is selected, ties to the smaller pool position j (for a pool
 *              that comes sorted from top-K: the higher score, then the smaller id).
 *   output     ids[u, t] / scores[u, t] = pool_ids / pool_scores of the t-th selected entry -- the original relevance score, not v, so the scores of
 *              a list need not descend.  Fewer than K valid entries: the remaining slots are id 0 / -inf, as in every top-K entry.
 *   ild[u]     (intra-list diversity) = the mean of 1 - c(i, j) over the unordered pairs of selected entries, 0 with fewer than two.  NULL: not wanted.
 * lambda = 1 selects the first K valid pool positions: on a top-K output, that output cut to K, bit for bit.
 * In fp32: <.,.> is the gather-and-dot of a4r_topk_lists (a lane's E / 16 products in sequence by fma, then a four-step butterfly over the row's 16
 * lanes), so c(i, j) is a pure function of the two rows, the same bits in every call, round and pool position, and c(i, j) = c(j, i); sqrt and
 * the divisions are correctly rounded (no reciprocal approximations); r is the fp64 quotient rounded once to fp32 (a score range beyond fp32's
 * cannot overflow it).  Where every quantity is exact in fp32 the result is the rule's.  The table rows are expected finite with a squared norm
 * that fp32 holds.
 * One launch, one 256-thread workgroup per user, an entry per thread; no workspace, no atomics, nothing written but the outputs.  Any NULL pointer but
 * ild, U < 1, N1 < 2, E outside {64, 128, 256, 512}, P outside 1 .. A4R_MMR_MAX_POOL, K outside 1 .. P, lambda outside [0, 1] or NaN, or item_emb not
 * 16-byte aligned: A4R_EINVAL before any HIP call. */
#define A4R_MMR_MAX_POOL 256          /* = A4R_TOPK_MAX_K: the pool is a top-K output */
int a4r_mmr_rerank(void* stream, const float* item_emb, const int32_t* pool_ids, const float* pool_scores,
                   int32_t* ids, float* scores, float* ild, float lambda, int U, int N1, int E, int P, int K);

#ifdef __cplusplus
}
#endif
#endif
