/* liba4r_hip.so: similar items -- every query item's K nearest items of the table, by cosine or by dot product.  Part of the C ABI of include/a4r.h,
 * which includes this file (new exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_similar.py, whose signature
 * table tests/test_similar_cpu.py holds against the prototypes below.  The rule is restated in fp64 in tests/similar_ref.py. */
#ifndef A4R_SIMILAR_H
#define A4R_SIMILAR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* a4r_row_inv_norms: inv[i] = fp32( 1 / sqrt( sum over e of (double)table[i][e]^2 ) ) for every row i < N1 of table (fp32 [N1, E]), row 0 included;
 * inv[i] = 0 when that sum is 0 or not finite (a zero row, or a row holding inf or NaN).  The squares are summed in fp64 (16 lanes per row, E / 16
 * elements per lane in sequence, then a four-step butterfly: no atomics, the same bits in every call); sqrt and the division are fp64, the result
 * is rounded to fp32 once.  One launch.  A NULL table or inv, N1 < 1, E outside {64, 128, 256, 512} or a table that is not 16-byte aligned:
 * A4R_EINVAL before any HIP call. */
int a4r_row_inv_norms(void* stream, const float* table, float* inv, int N1, int E);

/* a4r_topk_similar: for each of the Q query items query[r] (int32 [Q], ids of table rows), the K best other items of item_emb (fp32 [N1, E], row 0 =
 * the pad row) into ids int32 [Q, K] / scores fp32 [Q, K].
 *   score      dot metric (inv_norm NULL): score(q, i) = <item_emb[q], item_emb[i]>, formed by the item-table score sweep as a4r_topk_items forms
 *              <prec[u], item_emb[i]> -- the same fragments and MFMA chain, hence the same bits as a4r_topk_items with prec = item_emb[q].
 *              cosine metric (inv_norm = the fp32 [N1] output of a4r_row_inv_norms): score(q, i) = dot * (inv_norm[q] * inv_norm[i]) -- two fp32
 *              multiplies, the product of the two inverse norms formed first.  The sweep's dot depends on the two rows only and is symmetric,
 *              and the product commutes, so score(i, j) and score(j, i) are the same bits.  The score is not clamped: it may exceed 1 by a few ulps.
 *   never listed   row 0; the query itself (i == q: another row with the same content is listed); an item with cand[i] == 0 (cand uint8 [N1] as in
 *              include/a4r_candidates.h, NULL = no restriction; the query need not be a candidate); in cosine mode an item with inv_norm[i] == 0;
 *              an item whose score is not >= min_sim, compared on the score's own fp32 bits (-inf = no floor; a NaN score is never listed).
 *   pad lists  a query id outside 1 .. N1-1 gets a list of pads (id 0 / -inf) and no table row is read for it; so does, in cosine mode, a query with
 *              inv_norm[q] == 0.  Repeated query ids are independent rows with equal lists.
 *   order      score descending, ties to the smaller id (the key of a4r_topk_items); short lists end in pads (id 0 / -inf); -0 is returned as +0.
 *              Keys are a total order, so the result is unique and does not depend on the grid.
 * ws: a4r_topk_ws_bytes(Q, N1, K) bytes of device scratch, 8-byte aligned (the grid rule of a4r_topk_items with U = Q; contents need not be kept).
 * Two launches: per-range partial top-K, then a4r_topk_items' own merge (or decode, with one item range).  No atomics in global memory.
 * A NULL item_emb / query / ids / scores / ws, E outside {64, 128, 256, 512}, K outside 1 .. A4R_TOPK_MAX_K, Q < 1, N1 < 2, item_emb not 16-byte
 * aligned, ws not 8-byte aligned, or min_sim NaN: A4R_EINVAL before any HIP call. */
int a4r_topk_similar(void* stream, const float* item_emb, const float* inv_norm, const int32_t* query, const uint8_t* cand,
                     float min_sim, int32_t* ids, float* scores, void* ws, int Q, int N1, int E, int K);

#ifdef __cplusplus
}
#endif
#endif
