/* liba4r_hip.so: the negatives of a sampled evaluation drawn on the device.  Part of the C ABI of include/a4r.h, which includes this file (new
 * exports, ABI 411 kept: no existing argument list changes); bound by adapter4rec_amd/_lib_eval_negatives.py, whose signature table
 * tests/test_eval_negatives_cpu.py holds against the prototypes below. */
#ifndef A4R_EVAL_NEGATIVES_H
#define A4R_EVAL_NEGATIVES_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The protocol of most SASRec / IDRec papers: the held-out item is ranked among N items drawn from those the user has not interacted with,
 * uniformly or by popularity.  The draw rule is integer-only and pinned bit for bit (tests/eval_neg_ref.py restates it in Python ints):
 *   D(u)   = the distinct ids in 1 .. N1-1 among the first A4R_EVAL_MAX_HISTORY ids of hist(u) (CSR as a4r_eval_rank's), together with
 *            target[u] if it is an item, ascending.
 *   cdf    = int64 [N1], cdf[0] = 0, cdf[i] = cnt[1] + ... + cnt[i] for occurrence counts cnt >= 0 (popularity sampling: an item of count 0 is
 *            never drawn); cdf == NULL is uniform sampling, cnt[i] = 1, cdf[i] = i, and no array is read.
 *   m      = cdf[N1-1] - sum of cnt[d] over d in D(u).
 *   draw j = 0 .. N-1 of user u with key uk = user_key[u] (the caller's GLOBAL user id, not the position in the batch):
 *            h = a4r_hash64(seed, A4R_EVAL_NEG_SITE, ((uint64_t)(uint32_t)uk << 16) | j)      (the counter hash of csrc/a4r_common.h)
 *            x = the high 64 bits of h * m
 *            for every s in D(u) ascending: if (x >= cdf[s-1]) x += cnt[s]
 *            id = the smallest i with cdf[i] > x                                               (uniform: x + 1)
 *            (the kernels replace the walk by a binary search over the prefix masses of D(u); the ids are the same)
 *   The id is never a member of D(u), the pad row or an item of count 0.  A draw is a pure function of (seed, uk, j, D(u), cdf): the batch, its
 *   size and order, the rank, the epoch and the step do not enter.  Draws are independent (WITH replacement): an id can be drawn twice, the
 *   ranking counts it once (the rule of a4r_eval_rank_lists), so fewer than N distinct negatives may stand against the target.
 *   m < 1: the user has no candidate; all N draws are 0 (rank 1) and *err is incremented by one -- an integer atomic, the only one; *err is
 *   added to, never cleared: the caller zeroes it before the first call of an evaluation and reads it after the last.
 * a4r_eval_draw_negatives: out_ids int32 [U, N] = the draws.  One launch, one 256-thread workgroup per user.
 * a4r_eval_rank_sampled: rank[u] = 1 + #{distinct drawn i : score(u, i) > score(u, target[u])}, score exactly as in a4r_user_lists.h (the same fma
 *   sequence and 16-lane butterfly, the strict comparison on the ordered score half of the key, the same NaN rule): the rank a4r_eval_rank_lists
 *   gives on the materialised draws, from one launch that draws, gathers, scores and ranks with nothing of size U x N written to memory.  A target
 *   that is no item is never dereferenced and gets rank 1.
 * No workspace, no scratch, no float atomics, nothing written but rank / out_ids and *err.  Any NULL pointer but cdf (and the stream), U < 1,
 * N1 < 2, N outside 1 .. A4R_LIST_MAX, E outside {64, 128, 256, 512}, or prec / item_emb not 16-byte aligned: A4R_EINVAL before any HIP call. */
#define A4R_EVAL_NEG_SITE 7002
int a4r_eval_draw_negatives(void* stream, const int32_t* hist_ptr, const int32_t* hist_idx, const int32_t* target, const int32_t* user_key,
                            const int64_t* cdf, uint64_t seed, int32_t* out_ids, int32_t* err, int U, int N1, int N);
int a4r_eval_rank_sampled(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* hist_ptr,
                          const int32_t* hist_idx, const int32_t* user_key, const int64_t* cdf, uint64_t seed, int32_t* rank, int32_t* err,
                          int U, int N1, int E, int N);

#ifdef __cplusplus
}
#endif
#endif
