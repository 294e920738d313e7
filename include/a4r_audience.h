/* liba4r_hip.so: audience lists -- every query item's K best users of a user table, a user left out when the item is in the user's own seen list.
 * Part of the C ABI of include/a4r.h, which includes this file (a new export, ABI 411 kept: no existing argument list changes); bound by
 * adapter4rec_amd/_lib_audience.py, whose signature table tests/test_audience_cpu.py holds against the prototype below.  The rule is restated in
 * fp64 in tests/audience_ref.py. */
#ifndef A4R_AUDIENCE_H
#define A4R_AUDIENCE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* a4r_topk_users: for each of the Q query items query[r] (int32 [Q], ids of item_emb rows; item_emb fp32 [N1, E]), the K best rows of user_vec
 * (fp32 [U1, E], row 0 = a pad row: never read, never listed) into rows int32 [Q, K] / scores fp32 [Q, K].
 *   score      score(q, r) = <item_emb[q], user_vec[r]>, formed by the item-table score sweep with user_vec in the table's place and the 16 query
 *              rows of a workgroup loaded straight from item_emb[query[..]] -- the fragments and MFMA chain of a4r_topk_items, hence the bits of
 *              a4r_topk_items(prec = item_emb[query], item_emb := user_vec), and of the score a4r_topk_items gives the same (user, item) pair
 *              with the roles the usual way round.
 *   never listed   row 0; a row with elig[r] == 0 (elig uint8 [U1], NULL = no restriction); a row r whose seen list contains the query's id.
 *   seen lists     the seen list of row r is seen_idx[seen_ptr[r] .. seen_ptr[r + 1]): seen_ptr int64 [U1 + 1], non-decreasing, inside seen_idx
 *              (the caller's contract); seen_idx int32, ascending within a row.  Repeats are allowed; ids outside 1 .. N1-1 are harmless (no
 *              query has them); a list given for row 0 is never read.  There is no cap on a list's length: the lists stay in global memory.
 *   exclusion search   a key that beats its query's threshold is searched for in the row's seen list by binary search in global memory; the elig
 *              byte is tested ahead of the search.  The search never reads outside [seen_ptr[r], seen_ptr[r + 1]): an unsorted list can cause a
 *              wrong listing but never a stray read.
 *   pad lists  a query id outside 1 .. N1-1 gets a list of pads (row 0 / -inf) and no item_emb row is read for it.  Repeated query ids are
 *              independent rows with equal lists.
 *   order      score descending, ties to the smaller row (the key of a4r_topk_items); short lists end in pads (row 0 / -inf); -0 is returned as
 *              +0.  Keys are a total order, so the result is unique and does not depend on the grid.
 * ws: a4r_topk_ws_bytes(Q, U1, K) bytes of device scratch, 8-byte aligned (the grid rule of a4r_topk_items with U = Q, N1 = U1; contents need not
 * be kept).  Two launches: per-range partial top-K, then a4r_topk_items' own merge (or decode, with one range of rows).  No atomics in global
 * memory.  A NULL item_emb / query / user_vec / seen_ptr / seen_idx / rows / scores / ws, E outside {64, 128, 256, 512}, K outside
 * 1 .. A4R_TOPK_MAX_K, Q < 1, N1 < 2, U1 < 2, item_emb or user_vec not 16-byte aligned, ws or seen_ptr not 8-byte aligned: A4R_EINVAL before
 * any HIP call. */
int a4r_topk_users(void* stream, const float* item_emb, const int32_t* query, const float* user_vec, const int64_t* seen_ptr,
                   const int32_t* seen_idx, const uint8_t* elig, int32_t* rows, float* scores, void* ws, int Q, int N1, int U1, int E, int K);

#ifdef __cplusplus
}
#endif
#endif
