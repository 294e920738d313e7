/* liba4r_hip.so: top-K recommendation with exclusion lists of any length -- a4r_topk_items / a4r_topk_items_cand with each user's list left in
 * global memory.  Part of the C ABI of include/a4r.h, which includes this file (a new export, ABI 411 kept: no existing argument list changes);
 * bound by adapter4rec_amd/_lib_exclude.py, whose signature table tests/test_exclude_cpu.py holds against the prototype below.  The rule is
 * restated in numpy in tests/exclude_ref.py. */
#ifndef A4R_EXCLUDE_H
#define A4R_EXCLUDE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* a4r_topk_items_excl: ids int32 [U, K] / scores fp32 [U, K] = the K best items 1 .. N1-1 of every user (prec fp32 [U, E], item_emb fp32
 * [N1, E], row 0 = the pad item), among the items with cand[i] != 0 (cand uint8 [N1], NULL = all items), user u never given an id of
 * excl_idx[excl_ptr[u] .. excl_ptr[u + 1]).  It is a4r_topk_items (cand NULL) / a4r_topk_items_cand word for word, except for where the
 * lists live and how long they may be.
 *   exclusion lists   excl_ptr int64 [U + 1], non-decreasing, inside excl_idx, 8-byte aligned (the caller's contract); excl_idx int32, ascending
 *              within a user.  There is no cap on a list's length: the lists stay in global memory (a4r_topk_items keeps 264 ids per user in
 *              LDS and sorts them itself).  Repeated ids, id 0 and ids outside 1 .. N1-1 are allowed and match nothing.
 *   exclusion search   a key that beats its user's threshold is tested against cand[i] first, then searched in the user's list by binary search
 *              in global memory.  The search never reads outside [excl_ptr[u], excl_ptr[u + 1]): an unsorted list can cause a wrong listing
 *              but never a stray read, nor a read of a neighbour's list.
 *   score      score(u, i) = <prec[u], item_emb[i]> by the fragments and the MFMA chain of a4r_topk_items, hence its bits: on lists both
 *              entries serve (ascending, at most 264 ids) ids and scores are those of a4r_topk_items / a4r_topk_items_cand bit for bit.
 *   order      score descending, ties to the smaller id; NaN sorts below -inf; -0 is returned as +0; short lists end in pads (id 0 / -inf);
 *              row 0 is never listed.  Keys are a total order, so the result is unique and does not depend on the grid.
 * ws: a4r_topk_ws_bytes(U, N1, K) bytes of device scratch, 8-byte aligned (contents need not be kept).  Two launches: per-range partial top-K,
 * then a4r_topk_items' own merge (or decode, with one item range).  No atomics in global memory, no float atomics anywhere.  A NULL prec /
 * item_emb / excl_ptr / excl_idx / ids / scores / ws, E outside {64, 128, 256, 512}, K outside 1 .. A4R_TOPK_MAX_K, U < 1, N1 < 2, prec or
 * item_emb not 16-byte aligned, ws or excl_ptr not 8-byte aligned: A4R_EINVAL before
 * any HIP call. */
int a4r_topk_items_excl(void* stream, const float* prec, const float* item_emb, const int64_t* excl_ptr, const int32_t* excl_idx,
                        const uint8_t* cand, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K);

#ifdef __cplusplus
}
#endif
#endif
