// Top-K recommendation: the K best items of every user, history excluded, without materialising the [users, items] score matrix.
//
// score(u, i) = <prec[u], item_emb[i]> comes from the item-table score sweep (a4r_score_sweep.h), fp32, 16 users per workgroup, requested one
// tile ahead.  a4r_eval_rank forms its scores by the same fragments and the same MFMA chain (its hot loop writes them out itself, a4r_eval.hip),
// hence the same bits: tests/test_topk_gpu.py holds the two against each other.
//
// Selection.  An item is a 64-bit key  orderable(score) << 32 | ~id : one unsigned compare orders by score descending, then id ascending (NaN maps
// below -inf, -0 onto +0; key 0 is "no item").  Every user keeps a candidate buffer in LDS and a threshold, the K-th best key the workgroup
// holds (0 until it holds K).  A key above the threshold is checked against the user's exclusion list (sorted in LDS once, a binary search: the
// check runs for threshold-beating items only, off the hot loop) and appended.  The 4 waves meet at a barrier once per step of 4 tiles; a step
// adds at most 64 keys per user, so when any buffer has less than 64 free slots left, all 16 buffers are sorted (bitonic, in LDS) and cut back
// to K, which raises the thresholds.  At the end of its range the workgroup writes its K best keys per user (sorted) to the workspace.
//
// Merge.  A second launch turns the gy sorted lists of a user into the final K: with one item range it decodes the list; with more, every
// listed key's final position is its position in its own list plus the number of keys above it in the others (binary searches in LDS; keys are
// unique, so positions are distinct).  Keys are a total order and each item range holds every item of the global top K that falls in it, so
// the result does not depend on the grid.
//
// Similar items (a4r_topk_similar, include/a4r_similar.h).  similar_partial_kernel is the same sweep and selection with the 16 rows of a workgroup
// taken from the item table itself; compaction, merge and decode are the ones above, shared as they are.  a4r_row_inv_norms lives here too.
//
// Audience lists (a4r_topk_users, include/a4r_audience.h).  audience_partial_kernel is the similar kernel's row set swept over the user table: the
// K best users of every query item, a user dropped when the item is in the user's own seen list (searched in global memory, no cap on its length).
//
// Exclusion lists of any length (a4r_topk_items_excl, include/a4r_exclude.h).  topk_excl_partial_kernel is topk_partial_kernel with the users'
// lists left in global memory behind int64 offsets, searched the audience kernel's way: no cap on a list's length, no sorting prologue.
//
// Where the pieces live.  The key, its decoding, the rank sort of an id list and the search of the sorted list: a4r_select.h, shared with the list
// kernels.  Here, one copy each for the three partial kernels (fp32, bf16, similar), which keep their own loads and MFMA chains:
// topk_append (with the trigger protocol), topk_step_end, topk_write_out and topk_compact; on the host topk_args_ok (every export's checks) and
// topk_finish (decode or merge).  The two kernels with exclusion lists write the sort and the search of
// a4r_select.h out: timed through the helpers they lost 0.4 - 1 % (profiles/LOG.md).
#include <initializer_list>
#include "a4r_score_sweep.h"
#include "a4r_select.h"
#include "../../include/a4r.h"

namespace {

constexpr int MAXX = A4R_EVAL_MAX_HISTORY;   // exclusion ids per user kept in LDS (the a4r_eval_rank bound)
constexpr int STEP_KEYS = 64;                // keys a step can add per user: 4 waves x 16 item columns
constexpr int MAX_RANGES = 32;               // item ranges per user: the merge holds gy x K <= 32 x 256 keys (64 KiB) in LDS

// topk_key / topk_emit, rank_sort_i32 / sorted_has: a4r_select.h (shared with a4r_lists.hip and a4r_eval_negatives.hip)

// Sort each of the 16 buffers (cap keys, cap a power of two) descending, entries past the count as 0; keep the best K, reset the thresholds.
__device__ void topk_compact(uint64_t* buf, int cap, int K, int32_t* cnt, uint64_t* thr) {
    const int tid = threadIdx.x, lc = __builtin_ctz(cap);
    for (int e = tid; e < 16 * cap; e += 256)
        if ((e & (cap - 1)) >= cnt[e >> lc]) buf[e] = 0;
    __syncthreads();
    for (int k = 2; k <= cap; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < 8 * cap; p += 256) {                      // 16 users x cap / 2 pairs
                const int ul = p >> (lc - 1), q = p & ((cap >> 1) - 1);
                const int a = 2 * q - (q & (j - 1)), b = a + j;
                uint64_t* row = buf + (ul << lc);
                const uint64_t x = row[a], y = row[b];
                if (((a & k) == 0) ? x < y : x > y) { row[a] = y; row[b] = x; }
            }
            __syncthreads();
        }
    if (tid < 16) {
        const int c = min(cnt[tid], K);
        cnt[tid] = c;
        thr[tid] = c == K ? buf[(tid << lc) + K - 1] : 0;
    }
    __syncthreads();
}

// The pieces the three partial kernels below are made of.  A row set is 16 rows (users, or query items) of a workgroup with their LDS: 16 buffers
// of cap keys, cnt[16] and thr_s[16].  A kernel with several row sets passes the
// first set's pointers; set rs is 16 rs rows further on.

// Append and trigger: the key goes to the next free slot of row ul's buffer (ul counts over all row sets).  Slot p < cap: a step adds at most
// STEP_KEYS keys per row, and whenever a step leaves a buffer with fewer than STEP_KEYS free slots its writer sets trig = s, on which the step's
// end (topk_step_end, behind the step's barrier) cuts every buffer back to K <= cap - STEP_KEYS keys.  trig needs no atomic: every writer of
// step s writes the same s, in front of the step's barrier; behind it every wave reads trig before it can write s + 1 -- or, if a fast wave does
// write s + 1 first, then no one wrote s, and the slow wave reads a value that is not s either way.  If some one wrote s, all waves meet in
// topk_compact's barriers before any goes on to step s + 1.  So trig == s is uniform over the workgroup.
__device__ __forceinline__ void topk_append(uint64_t* buf, int cap, int32_t* cnt, int& trig, int ul, uint64_t key, int s) {
    const int p = atomicAdd(&cnt[ul], 1);
    buf[ul * cap + p] = key;
    if (p >= cap - STEP_KEYS) trig = s;
}

// topk_compact for each of RS row sets.  (One set is written without the loop: through a loop of one trip the compiler computes what the calls
// share in front of the sweep and every fp32 kernel holds one more VGPR across it.)
template <int RS> __device__ __forceinline__ void topk_compact_sets(uint64_t* buf, int cap, int K, int32_t* cnt, uint64_t* thr_s) {
    if constexpr (RS == 1) topk_compact(buf, cap, K, cnt, thr_s);
    else
        for (int rs = 0; rs < RS; ++rs) topk_compact(buf + rs * 16 * cap, cap, K, cnt + rs * 16, thr_s + rs * 16);
}

// Behind step s's barrier: on the trigger, compact each of the N / 4 row sets and reload this lane's thresholds (thr[rs * 4 + rr]: row rs * 16 + kg * 4 + rr).
template <int N> __device__ __forceinline__ void topk_step_end(uint64_t* buf, int cap, int K, int32_t* cnt, uint64_t* thr_s, const int& trig, int s,
                                                               int kg, uint64_t (&thr)[N]) {
    if (trig != s) return;
    topk_compact_sets<N / 4>(buf, cap, K, cnt, thr_s);
#pragma unroll
    for (int m = 0; m < N; ++m) thr[m] = thr_s[(m >> 2) * 16 + kg * 4 + (m & 3)];
}

// End of the workgroup's item range: the final compaction, then the K best keys of each of its rows u0 .. (sorted) go to the workspace.
template <int RS> __device__ __forceinline__ void topk_write_out(uint64_t* buf, int cap, int K, int32_t* cnt, uint64_t* thr_s,
                                                                 uint64_t* __restrict__ ws, int u0, int U) {
    topk_compact_sets<RS>(buf, cap, K, cnt, thr_s);
    for (int e = threadIdx.x; e < 16 * RS * K; e += 256) {
        const int ul = e / K, j = e - ul * K;
        if (u0 + ul < U) ws[((size_t)blockIdx.y * U + u0 + ul) * K + j] = buf[ul * cap + j];
    }
}

// CAND (a4r_topk_items_cand, include/a4r_candidates.h): an item is kept only if cand[i] != 0 -- a byte per table row in global memory, tested
// beside the exclusion search, for threshold-beating items only.  CAND = false is the kernel as it was and never reads cand.
template <int E, bool CAND>
__global__ void __launch_bounds__(256) topk_partial_kernel(const float* __restrict__ prec, const float* __restrict__ item_emb,
                                                           const int32_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_idx,
                                                           uint64_t* __restrict__ ws, int U, int N1, int K, int cap,
                                                           const uint8_t* __restrict__ cand) {
    constexpr int KS = E / 16;                       // chunk steps (fp32: 16 k per step)
    constexpr int PER = (MAXX + 15) / 16;            // exclusion ids per thread while sorting
    extern __shared__ uint64_t buf[];                // [16][cap] candidate keys
    __shared__ int32_t excl[16][MAXX];
    __shared__ int32_t nex[16];
    __shared__ int32_t cnt[16];
    __shared__ uint64_t thr_s[16];
    __shared__ int trig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * 16;
    {   // 16 threads per user copy its exclusion ids and sort them: rank_sort_i32 (a4r_select.h) written out -- through it, or through a helper
        // around this block, the kernel ran 0.5 % slower at K = 100 with equal registers (profiles/LOG.md)
        const int ul = tid >> 4, j0 = tid & 15, u = min(u0 + ul, U - 1);
        const int b = excl_ptr[u], n = max(0, min(excl_ptr[u + 1] - b, MAXX));
        for (int j = j0; j < n; j += 16) excl[ul][j] = excl_idx[b + j];
        if (j0 == 0) { nex[ul] = n; cnt[ul] = 0; thr_s[ul] = 0; }
        if (tid == 0) trig = -1;
        __syncthreads();
        int v[PER], pos[PER];
#pragma unroll
        for (int m = 0; m < PER; ++m) {
            const int j = j0 + 16 * m;
            pos[m] = -1; v[m] = 0;
            if (j < n) {
                const int x = excl[ul][j];
                int p = 0;
                for (int k = 0; k < n; ++k) {
                    const int y = excl[ul][k];
                    p += (y < x || (y == x && k < j)) ? 1 : 0;
                }
                v[m] = x; pos[m] = p;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < PER; ++m)
            if (pos[m] >= 0) excl[ul][pos[m]] = v[m];
    }
    uint4 ua[KS];                                    // A operand: the 16 users
    frag_load<E>(ua, prec, min(u0 + r16, U - 1), kg);
    __syncthreads();
    const SweepDeal<> deal(N1, wave);
    const int nsteps = deal.steps();                 // the 4 waves meet at every step's barrier
    uint64_t thr[4] = {0, 0, 0, 0};
    bool live[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) live[rr] = u0 + kg * 4 + rr < U;
    int t = deal.first;
    uint4 bn[KS];
    sweep_begin<E, true>(bn, item_emb, deal, r16, kg);
    for (int s = 0; s < nsteps; ++s, t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column (>= N1 past the end of the table: nothing to add)
        uint4 b[KS];
        sweep_next<E, true>(b, bn, item_emb, deal, t, r16, kg);
        const f32x4_t acc = score_tile<float>(ua, b);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const uint64_t key = topk_key(acc[rr], i);
            if (i < N1 && live[rr] && key > thr[rr]) {
                if constexpr (CAND)
                    if (cand[i] == 0) continue;              // (ahead of the search: under a sparse mask the thresholds stay low for long)
                const int ul = kg * 4 + rr;
                int lo = 0, hi = nex[ul];                    // sorted_has written out: through it another 0.5 % at K = 100 (profiles/LOG.md)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (excl[ul][mid] < i) lo = mid + 1; else hi = mid;
                }
                if (!(lo < nex[ul] && excl[ul][lo] == i)) {
                    topk_append(buf, cap, cnt, trig, ul, key, s);
                }
            }
        }
        __syncthreads();
        topk_step_end(buf, cap, K, cnt, thr_s, trig, s, kg, thr);
    }
    topk_write_out<1>(buf, cap, K, cnt, thr_s, ws, u0, U);
}

// Exclusion lists of any length (a4r_topk_items_excl, include/a4r_exclude.h): topk_partial_kernel with the users' lists left in global memory.
// The LDS list, its count and the sorting prologue are gone; the lists come ascending (the caller's contract) behind int64 offsets.  The 16
// users' two offsets are loaded once into LDS (256 B) -- they do not change with the column, so the sweep loads none -- and a key that beats its
// threshold is searched in excl_idx[b .. e) by audience_partial_kernel's bisection, behind the cand byte under CAND.  lo <= mid < hi <= e
// throughout: every read lies inside the user's own list, so an unsorted list can mislist but never strays into a neighbour's.
template <int E, bool CAND>
__global__ void __launch_bounds__(256) topk_excl_partial_kernel(const float* __restrict__ prec, const float* __restrict__ item_emb,
                                                                const int64_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_idx,
                                                                uint64_t* __restrict__ ws, int U, int N1, int K, int cap,
                                                                const uint8_t* __restrict__ cand) {
    constexpr int KS = E / 16;                       // chunk steps (fp32: 16 k per step)
    extern __shared__ uint64_t buf[];                // [16][cap] candidate keys
    __shared__ int64_t xb[16], xe[16];               // the users' lists: excl_idx[xb[ul] .. xe[ul])
    __shared__ int32_t cnt[16];
    __shared__ uint64_t thr_s[16];
    __shared__ int trig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * 16;
    if (tid < 16) {
        const int u = min(u0 + tid, U - 1);
        xb[tid] = excl_ptr[u]; xe[tid] = excl_ptr[u + 1];
        cnt[tid] = 0; thr_s[tid] = 0;
    }
    if (tid == 0) trig = -1;
    uint4 ua[KS];                                    // A operand: the 16 users
    frag_load<E>(ua, prec, min(u0 + r16, U - 1), kg);
    __syncthreads();
    const SweepDeal<> deal(N1, wave);
    const int nsteps = deal.steps();                 // the 4 waves meet at every step's barrier
    uint64_t thr[4] = {0, 0, 0, 0};
    bool live[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) live[rr] = u0 + kg * 4 + rr < U;
    int t = deal.first;
    uint4 bn[KS];
    sweep_begin<E, true>(bn, item_emb, deal, r16, kg);
    for (int s = 0; s < nsteps; ++s, t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column (>= N1 past the end of the table: nothing to add)
        uint4 b[KS];
        sweep_next<E, true>(b, bn, item_emb, deal, t, r16, kg);
        const f32x4_t acc = score_tile<float>(ua, b);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const uint64_t key = topk_key(acc[rr], i);
            if (i < N1 && live[rr] && key > thr[rr]) {
                if constexpr (CAND)
                    if (cand[i] == 0) continue;              // (ahead of the search: under a sparse mask the thresholds stay low for long)
                const int ul = kg * 4 + rr;
                const int64_t le = xe[ul];
                int64_t lo = xb[ul], hi = le;                // lo <= mid < hi <= le throughout: every read lies inside the user's own list
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (excl_idx[mid] < i) lo = mid + 1; else hi = mid;
                }
                if (!(lo < le && excl_idx[lo] == i)) topk_append(buf, cap, cnt, trig, ul, key, s);
            }
        }
        __syncthreads();
        topk_step_end(buf, cap, K, cnt, thr_s, trig, s, kg, thr);
    }
    topk_write_out<1>(buf, cap, K, cnt, thr_s, ws, u0, U);
}

// Scores from the bf16 MFMA (a4r_topk_items_bf16, include/a4r_score_bf16.h): topk_partial_kernel at prec_b = bf16(prec), table_b = bf16(item_emb),
// the scores by eval_rank_bf16_kernel's chain (score_tile<bf16_t>), so the two entries give the same bits.  A workgroup holds RS sets of 16 users:
// the A fragments, the buffer, the threshold, counter and exclusion arrays are 16 RS users wide, a table tile is loaded once for all of them, and
// PD tiles are in flight per wave (the ring of eval_rank_bf16_kernel).  A step still adds at most STEP_KEYS keys per USER, so cap, the trigger and
// topk_compact -- called once per row set on that set's 16 buffers -- are as above; so are the key, the merge and the decode.
template <int E, int RS, int PD, bool CAND>
__global__ void __launch_bounds__(256) topk_partial_bf16_kernel(const bf16_t* __restrict__ prec, const bf16_t* __restrict__ table,
                                                                const int32_t* __restrict__ excl_ptr, const int32_t* __restrict__ excl_idx,
                                                                uint64_t* __restrict__ ws, int U, int N1, int K, int cap,
                                                                const uint8_t* __restrict__ cand) {
    constexpr int KS = E / 32;                       // chunk steps (bf16: 32 k per step)
    constexpr int PER = (MAXX + 15) / 16;            // exclusion ids per thread while sorting
    constexpr int R = 16 * RS;                       // users of a workgroup
    extern __shared__ uint64_t buf[];                // [R][cap] candidate keys
    __shared__ int32_t excl[R][MAXX];
    __shared__ int32_t nex[R];
    __shared__ int32_t cnt[R];
    __shared__ uint64_t thr_s[R];
    __shared__ int trig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * R;
    if (tid == 0) trig = -1;
    for (int rs = 0; rs < RS; ++rs) {   // as in topk_partial_kernel, one row set at a time (the sets' rows are disjoint); written out for its reason: 0.4 - 0.6 % at K = 10
        const int ul = rs * 16 + (tid >> 4), j0 = tid & 15, u = min(u0 + ul, U - 1);
        const int b = excl_ptr[u], n = max(0, min(excl_ptr[u + 1] - b, MAXX));
        for (int j = j0; j < n; j += 16) excl[ul][j] = excl_idx[b + j];
        if (j0 == 0) { nex[ul] = n; cnt[ul] = 0; thr_s[ul] = 0; }
        __syncthreads();
        int v[PER], pos[PER];
#pragma unroll
        for (int m = 0; m < PER; ++m) {
            const int j = j0 + 16 * m;
            pos[m] = -1; v[m] = 0;
            if (j < n) {
                const int x = excl[ul][j];
                int p = 0;
                for (int k = 0; k < n; ++k) {
                    const int y = excl[ul][k];
                    p += (y < x || (y == x && k < j)) ? 1 : 0;
                }
                v[m] = x; pos[m] = p;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < PER; ++m)
            if (pos[m] >= 0) excl[ul][pos[m]] = v[m];
    }
    uint4 ua[RS][KS];                                // A operand: RS sets of 16 users
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) frag_load<E>(ua[rs], prec, min(u0 + rs * 16 + r16, U - 1), kg);
    __syncthreads();
    const SweepDeal<> deal(N1, wave);
    const int nsteps = deal.steps();                 // the 4 waves meet at every step's barrier
    uint64_t thr[4 * RS];                            // [rs][rr]
    bool live[RS][4];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) { thr[rs * 4 + rr] = 0; live[rs][rr] = u0 + rs * 16 + kg * 4 + rr < U; }
    uint4 bn[PD][KS];
#pragma unroll
    for (int j = 0; j < PD; ++j) frag_load<E>(bn[j], table, deal.row(deal.first + j * deal.tstep, r16), kg);
    for (int sb = 0; sb < nsteps; sb += PD) {
#pragma unroll
        for (int j = 0; j < PD; ++j) {
            const int s = sb + j;
            if (s < nsteps) {                             // uniform over the workgroup
                const int t = deal.first + s * deal.tstep;
                const int i = 1 + t * 16 + r16;           // this lane's item column (>= N1 past the end of the table: nothing to add)
                uint4 b[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) b[ks] = bn[j][ks];
                frag_load<E>(bn[j], table, deal.row(t + PD * deal.tstep, r16), kg);
#pragma unroll
                for (int rs = 0; rs < RS; ++rs) {
                    const f32x4_t acc = score_tile<bf16_t>(ua[rs], b);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const uint64_t key = topk_key(acc[rr], i);
                        if (i < N1 && live[rs][rr] && key > thr[rs * 4 + rr]) {
                            if constexpr (CAND)
                                if (cand[i] == 0) continue;
                            const int ul = rs * 16 + kg * 4 + rr;
                            int lo = 0, hi = nex[ul];
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                if (excl[ul][mid] < i) lo = mid + 1; else hi = mid;
                            }
                            if (!(lo < nex[ul] && excl[ul][lo] == i)) {
                                topk_append(buf, cap, cnt, trig, ul, key, s);
                            }
                        }
                    }
                }
                __syncthreads();
                topk_step_end(buf, cap, K, cnt, thr_s, trig, s, kg, thr);
            }
        }
    }
    topk_write_out<RS>(buf, cap, K, cnt, thr_s, ws, u0, U);
}

// Similar items (a4r_topk_similar, include/a4r_similar.h): topk_partial_kernel with the 16 rows of a workgroup taken from the table itself.  The A
// fragments are loaded straight from item_emb[query[..]] (no gather); one compare i == q stands where the exclusion list, its LDS and its sorting
// prologue were.  COS is the cosine metric (inv non-null): score = dot * (inv[q] * inv[i]); inv[i] of the lane's item column is requested with that
// tile's fragments, one tile ahead, and the inv[q] of the lane's four accumulator rows stay in registers.  A row whose query id is no item
// (or has inv[q] == 0) is dead: it adds no key, and its fragments come from row 0.
template <int E, bool CAND, bool COS>
__global__ void __launch_bounds__(256) similar_partial_kernel(const float* __restrict__ item_emb, const float* __restrict__ inv,
                                                              const int32_t* __restrict__ query, const uint8_t* __restrict__ cand, float min_sim,
                                                              uint64_t* __restrict__ ws, int Q, int N1, int K, int cap) {
    constexpr int KS = E / 16;
    extern __shared__ uint64_t buf[];                // [16][cap] candidate keys
    __shared__ int32_t cnt[16];
    __shared__ uint64_t thr_s[16];
    __shared__ int trig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * 16;
    constexpr bool cosine = COS;                     // (a template argument: as a run-time branch beside the request-ahead loads it cost 15 - 60 registers)
    if (tid < 16) { cnt[tid] = 0; thr_s[tid] = 0; }
    if (tid == 0) trig = -1;
    uint4 ua[KS];                                    // A operand: the 16 query rows
    {
        const int q = query[min(u0 + r16, Q - 1)];
        frag_load<E>(ua, item_emb, (q >= 1 && q < N1) ? q : 0, kg);
    }
    int qid[4];                                      // the query ids of this lane's accumulator rows, 0 = dead
    float iq[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = u0 + kg * 4 + rr;
        const int q = query[min(r, Q - 1)];
        const bool ok = r < Q && q >= 1 && q < N1;
        iq[rr] = (ok && cosine) ? inv[q] : 1.f;
        qid[rr] = (ok && iq[rr] != 0.f) ? q : 0;
    }
    __syncthreads();
    const SweepDeal<> deal(N1, wave);
    const int nsteps = deal.steps();                 // the 4 waves meet at every step's barrier
    uint64_t thr[4] = {0, 0, 0, 0};
    int t = deal.first;
    uint4 bn[KS];
    sweep_begin<E, true>(bn, item_emb, deal, r16, kg);
    float ivn = cosine ? inv[deal.row(deal.first, r16)] : 1.f;
    for (int s = 0; s < nsteps; ++s, t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column (>= N1 past the end of the table: nothing to add)
        uint4 b[KS];
        const float iv = ivn;
        sweep_next<E, true>(b, bn, item_emb, deal, t, r16, kg);
        if (cosine) ivn = inv[deal.row(t + deal.tstep, r16)];
        const f32x4_t acc = score_tile<float>(ua, b);
        const bool col = i < N1 && iv != 0.f;           // (dot metric: iv = 1)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float sc = cosine ? acc[rr] * (iq[rr] * iv) : acc[rr];
            const uint64_t key = topk_key(sc, i);
            if (col && qid[rr] != 0 && i != qid[rr] && sc >= min_sim && key > thr[rr]) {
                if constexpr (CAND)
                    if (cand[i] == 0) continue;
                topk_append(buf, cap, cnt, trig, kg * 4 + rr, key, s);
            }
        }
        __syncthreads();
        topk_step_end(buf, cap, K, cnt, thr_s, trig, s, kg, thr);
    }
    topk_write_out<1>(buf, cap, K, cnt, thr_s, ws, u0, Q);
}

// Audience lists (a4r_topk_users, include/a4r_audience.h): similar_partial_kernel's row set -- the A fragments straight from item_emb[query[..]] --
// swept over the USER table, with the exclusion on the table side: row i is dropped for query q when q is in row i's own seen list
// seen_idx[seen_ptr[i] .. seen_ptr[i + 1]).  The lists stay in global memory, whatever their length, and are read for threshold-beating keys only:
// a lane whose column has such a key tests elig[i] (ELIG), loads the row's two offsets once for its four accumulator rows, and searches the list
// for each beating row's query id.  lo and mid stay inside [b, e) whatever the list holds, so an unsorted list can mislist but never strays.
// A row whose query id is no item is dead: it adds no key, its fragments are zero and no item_emb row is read for it.
template <int E, bool ELIG>
__global__ void __launch_bounds__(256) audience_partial_kernel(const float* __restrict__ item_emb, const int32_t* __restrict__ query,
                                                               const float* __restrict__ user_vec, const int64_t* __restrict__ seen_ptr,
                                                               const int32_t* __restrict__ seen_idx, const uint8_t* __restrict__ elig,
                                                               uint64_t* __restrict__ ws, int Q, int N1, int U1, int K, int cap) {
    constexpr int KS = E / 16;
    extern __shared__ uint64_t buf[];                // [16][cap] candidate keys
    __shared__ int32_t cnt[16];
    __shared__ uint64_t thr_s[16];
    __shared__ int trig;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * 16;
    if (tid < 16) { cnt[tid] = 0; thr_s[tid] = 0; }
    if (tid == 0) trig = -1;
    uint4 ua[KS];                                    // A operand: the 16 query items' rows
    {
        const int q = query[min(u0 + r16, Q - 1)];
        if (q >= 1 && q < N1) frag_load<E>(ua, item_emb, q, kg);
        else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) ua[ks] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    int qid[4];                                      // the query ids of this lane's accumulator rows, 0 = dead
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = u0 + kg * 4 + rr;
        const int q = query[min(r, Q - 1)];
        qid[rr] = (r < Q && q >= 1 && q < N1) ? q : 0;
    }
    __syncthreads();
    const SweepDeal<> deal(U1, wave);
    const int nsteps = deal.steps();                 // the 4 waves meet at every step's barrier
    uint64_t thr[4] = {0, 0, 0, 0};
    int t = deal.first;
    uint4 bn[KS];
    sweep_begin<E, true>(bn, user_vec, deal, r16, kg);
    for (int s = 0; s < nsteps; ++s, t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's user row (>= U1 past the end of the table: nothing to add)
        uint4 b[KS];
        sweep_next<E, true>(b, bn, user_vec, deal, t, r16, kg);
        const f32x4_t acc = score_tile<float>(ua, b);
        uint64_t key[4];
        bool any = false;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            key[rr] = topk_key(acc[rr], i);
            if (!(i < U1 && qid[rr] != 0 && key[rr] > thr[rr])) key[rr] = 0;      // (a live key is never 0)
            any |= key[rr] != 0;
        }
        bool open = any;
        if constexpr (ELIG)
            if (any) open = elig[i] != 0;               // (ahead of the search: under a sparse mask the thresholds stay low for long)
        if (open) {
            const int64_t lb = seen_ptr[i], le = seen_ptr[i + 1];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                if (key[rr] == 0) continue;
                int64_t lo = lb, hi = le;               // lo <= mid < hi <= le throughout: every read lies inside the row's own list
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (seen_idx[mid] < qid[rr]) lo = mid + 1; else hi = mid;
                }
                if (!(lo < le && seen_idx[lo] == qid[rr])) topk_append(buf, cap, cnt, trig, kg * 4 + rr, key[rr], s);
            }
        }
        __syncthreads();
        topk_step_end(buf, cap, K, cnt, thr_s, trig, s, kg, thr);
    }
    topk_write_out<1>(buf, cap, K, cnt, thr_s, ws, u0, Q);
}

// a4r_row_inv_norms: 16 lanes per row; a lane squares and sums its 16-byte chunks j, j + 16, ... in fp64, then a butterfly over the row's lanes
template <int E>
__global__ void __launch_bounds__(256) row_inv_norms_kernel(const float* __restrict__ table, float* __restrict__ inv, int N1) {
    const int j = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t r = row < N1 ? row : N1 - 1;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < E / 64; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(table + r * E + (c * 16 + j) * 4);
        s += (double)v.x * (double)v.x;
        s += (double)v.y * (double)v.y;
        s += (double)v.z * (double)v.z;
        s += (double)v.w * (double)v.w;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (j == 0 && row < N1) inv[row] = (s > 0.0 && s < __builtin_huge_val()) ? (float)(1.0 / sqrt(s)) : 0.f;      // (NaN fails both compares)
}

// one item range: the workgroup's sorted list is the answer
__global__ void topk_decode_kernel(const uint64_t* __restrict__ ws, int32_t* __restrict__ ids, float* __restrict__ scores, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) topk_emit(ws[e], ids + e, scores + e);
}

// gy > 1 item ranges: one workgroup per user; list l of user u is ws[(l * U + u) * K ..][K], sorted descending
__global__ void __launch_bounds__(256) topk_merge_kernel(const uint64_t* __restrict__ ws, int32_t* __restrict__ ids, float* __restrict__ scores,
                                                         int U, int K, int gy) {
    extern __shared__ uint64_t lists[];              // [gy][K]
    const int u = blockIdx.x, tid = threadIdx.x, n = gy * K;
    for (int e = tid; e < n; e += 256) {
        const int l = e / K, j = e - l * K;
        lists[e] = ws[((size_t)l * U + u) * K + j];
    }
    for (int j = tid; j < K; j += 256) topk_emit(0, ids + (size_t)u * K + j, scores + (size_t)u * K + j);    // pads; overwritten below where a key lands
    __syncthreads();                                  // (also orders the pad stores before the stores below: one workgroup)
    for (int e = tid; e < n; e += 256) {
        const uint64_t x = lists[e];
        if (x == 0) continue;
        const int l = e / K;
        int r = e - l * K;
        for (int m = 0; m < gy && r < K; ++m) {
            if (m == l) continue;
            const uint64_t* L = lists + m * K;
            int lo = 0, hi = K;                       // keys of list m above x: the first position holding a key <= x
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (L[mid] > x) lo = mid + 1; else hi = mid;
            }
            r += lo;
        }
        if (r < K) topk_emit(x, ids + (size_t)u * K + r, scores + (size_t)u * K + r);
    }
}

int topk_ranges(int U, int N1, int rs = 1) {         // a4r_eval_rank's grid over workgroups of 16 rs users, at most MAX_RANGES item ranges
    const int gy = sweep_ranges((U + rs - 1) / rs, N1);
    return gy < MAX_RANGES ? gy : MAX_RANGES;
}

int topk_cap(int K) {                                // candidate slots per user: a power of two >= K + one step's keys
    int c = 128;
    while (c < K + STEP_KEYS) c <<= 1;
    return c;
}

bool topk_shape_ok(int U, int N1, int K) { return U > 0 && N1 >= 2 && K >= 1 && K <= A4R_TOPK_MAX_K; }

// What every export checks in front of its first HIP call: the pointers it requires (the optional ones, cand and inv_norm, are its own business)
// and the workspace non-null, a shape and a width that are served, 16-byte operands a and b (b NULL: one operand), an 8-byte workspace.
bool topk_args_ok(std::initializer_list<const void*> required, const void* a, const void* b, const void* ws, int rows, int N1, int E, int K) {
    for (const void* p : required)
        if (!p) return false;
    return ws && topk_shape_ok(rows, N1, K) && width_served(WidthsF32{}, E) && aligned16(a, b) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0;
}

// The second launch of every export, behind its partial kernel: one item range is decoded, more are merged.  -> the launch status of both.
int topk_finish(hipStream_t s, const uint64_t* ws, int32_t* ids, float* scores, int rows, int K, int gy) {
    if (gy == 1) {
        const int64_t n = (int64_t)rows * K;
        const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
        hipLaunchKernelGGL(topk_decode_kernel, dim3(blocks), dim3(256), 0, s, ws, ids, scores, n);
    } else {
        const size_t mlds = (size_t)gy * K * sizeof(uint64_t);
        if (int rc = a4r_set_lds(topk_merge_kernel, mlds)) return rc;
        hipLaunchKernelGGL(topk_merge_kernel, dim3(rows), dim3(256), mlds, s, ws, ids, scores, rows, K, gy);
    }
    return a4r_launch_status();
}

// the one launch path of a4r_topk_items and a4r_topk_items_cand; cand is read by the CAND = true kernels only
template <bool CAND>
int topk_launch(void* stream, const float* prec, const float* item_emb, const int32_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand,
                int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K) {
    if (!topk_args_ok({prec, item_emb, excl_ptr, excl_idx, ids, scores}, prec, item_emb, ws, U, N1, E, K) || (CAND && !cand)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t* w = static_cast<uint64_t*>(ws);
    const int gy = topk_ranges(U, N1), cap = topk_cap(K);
    const dim3 grid((U + 15) / 16, gy);
    const size_t lds = (size_t)16 * cap * sizeof(uint64_t);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        const auto kernel = topk_partial_kernel<decltype(e)::value, CAND>;
        if ((rc = a4r_set_lds(kernel, lds))) return;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, prec, item_emb, excl_ptr, excl_idx, w, U, N1, K, cap, cand);
    });
    return rc ? rc : topk_finish(s, w, ids, scores, U, K, gy);
}

// a4r_topk_items_excl's launches: topk_launch's grid, capacity and finish behind the kernel that leaves the lists in global memory
template <bool CAND>
int topk_excl_launch(hipStream_t s, const float* prec, const float* item_emb, const int64_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand,
                     int32_t* ids, float* scores, uint64_t* w, int U, int N1, int E, int K) {
    const int gy = topk_ranges(U, N1), cap = topk_cap(K);
    const dim3 grid((U + 15) / 16, gy);
    const size_t lds = (size_t)16 * cap * sizeof(uint64_t);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        const auto kernel = topk_excl_partial_kernel<decltype(e)::value, CAND>;
        if ((rc = a4r_set_lds(kernel, lds))) return;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, prec, item_emb, excl_ptr, excl_idx, w, U, N1, K, cap, cand);
    });
    return rc ? rc : topk_finish(s, w, ids, scores, U, K, gy);
}

// Row sets of a4r_topk_items_bf16 per (E, K).  LDS bounds them: a row set is a 16-user buffer of 16 cap keys (16 / 32 / 64 KB at K <= 64 / <= 192 / <= 256)
// beside 17 KB of exclusion ids, so two sets at K <= 64 are 66 KB (two workgroups a CU) and two sets above are one workgroup a CU or none.  Timings
// choose within that: two sets at E = 128 / 256, where the table's bytes bind; one at E = 64, where the second set's LDS halves
// the workgroups a CU holds and the launch ran twice as long; one at E = 512, where the A fragments of two sets are 128 VGPRs beside the tiles.
int topk_bf16_rs(int E, int K) { return (K <= 64 && (E == 128 || E == 256)) ? 2 : 1; }
template <int E> struct TopkBf16Shape { static constexpr int PD = E == 64 ? 4 : E == 128 ? 2 : 1; };      // tiles in flight per wave

template <int E, int RS, bool CAND>
int topk_bf16_partial(hipStream_t s, const bf16_t* prec, const bf16_t* table, const int32_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand,
                      uint64_t* w, int U, int N1, int K, int gy) {
    const int cap = topk_cap(K);
    const dim3 grid((U + 16 * RS - 1) / (16 * RS), gy);
    const size_t lds = (size_t)16 * RS * cap * sizeof(uint64_t);
    const auto kernel = topk_partial_bf16_kernel<E, RS, TopkBf16Shape<E>::PD, CAND>;
    if (int rc = a4r_set_lds(kernel, lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, prec, table, excl_ptr, excl_idx, w, U, N1, K, cap, cand);
    return A4R_OK;
}

template <bool CAND>
int topk_bf16_launch(hipStream_t s, const bf16_t* prec, const bf16_t* table, const int32_t* excl_ptr, const int32_t* excl_idx, const uint8_t* cand,
                     int32_t* ids, float* scores, uint64_t* w, int U, int N1, int E, int K) {
    const int rs = topk_bf16_rs(E, K), gy = topk_ranges(U, N1, rs);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        if constexpr (W == 128 || W == 256) {
            if (rs == 2) { rc = topk_bf16_partial<W, 2, CAND>(s, prec, table, excl_ptr, excl_idx, cand, w, U, N1, K, gy); return; }
        }
        rc = topk_bf16_partial<W, 1, CAND>(s, prec, table, excl_ptr, excl_idx, cand, w, U, N1, K, gy);
    });
    return rc ? rc : topk_finish(s, w, ids, scores, U, K, gy);
}

// a4r_topk_similar's launches: the partial kernel above over top-K's grid with U = Q, then top-K's own decode or merge
template <bool CAND, bool COS>
int similar_launch(hipStream_t s, const float* item_emb, const float* inv, const int32_t* query, const uint8_t* cand, float min_sim, int32_t* ids,
                   float* scores, uint64_t* w, int Q, int N1, int E, int K) {
    const int gy = topk_ranges(Q, N1), cap = topk_cap(K);
    const dim3 grid((Q + 15) / 16, gy);
    const size_t lds = (size_t)16 * cap * sizeof(uint64_t);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        const auto kernel = similar_partial_kernel<decltype(e)::value, CAND, COS>;
        if ((rc = a4r_set_lds(kernel, lds))) return;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, item_emb, inv, query, cand, min_sim, w, Q, N1, K, cap);
    });
    return rc ? rc : topk_finish(s, w, ids, scores, Q, K, gy);
}

// a4r_topk_users' launches: the partial kernel above over top-K's grid with U = Q and the user table in the item table's place, then top-K's own
// decode or merge
template <bool ELIG>
int audience_launch(hipStream_t s, const float* item_emb, const int32_t* query, const float* user_vec, const int64_t* seen_ptr,
                    const int32_t* seen_idx, const uint8_t* elig, int32_t* rows, float* scores, uint64_t* w, int Q, int N1, int U1, int E, int K) {
    const int gy = topk_ranges(Q, U1), cap = topk_cap(K);
    const dim3 grid((Q + 15) / 16, gy);
    const size_t lds = (size_t)16 * cap * sizeof(uint64_t);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        const auto kernel = audience_partial_kernel<decltype(e)::value, ELIG>;
        if ((rc = a4r_set_lds(kernel, lds))) return;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, item_emb, query, user_vec, seen_ptr, seen_idx, elig, w, Q, N1, U1, K, cap);
    });
    return rc ? rc : topk_finish(s, w, rows, scores, Q, K, gy);
}

}  // namespace

extern "C" int a4r_topk_users(void* stream, const float* item_emb, const int32_t* query, const float* user_vec, const int64_t* seen_ptr,
                              const int32_t* seen_idx, const uint8_t* elig, int32_t* rows, float* scores, void* ws, int Q, int N1, int U1, int E,
                              int K) {
    if (!topk_args_ok({item_emb, query, user_vec, seen_ptr, seen_idx, rows, scores}, item_emb, user_vec, ws, Q, U1, E, K) || N1 < 2 ||
        (reinterpret_cast<uintptr_t>(seen_ptr) & 7u) != 0)
        return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t* w = static_cast<uint64_t*>(ws);
    return elig ? audience_launch<true>(s, item_emb, query, user_vec, seen_ptr, seen_idx, elig, rows, scores, w, Q, N1, U1, E, K)
                : audience_launch<false>(s, item_emb, query, user_vec, seen_ptr, seen_idx, nullptr, rows, scores, w, Q, N1, U1, E, K);
}

extern "C" int a4r_topk_items_excl(void* stream, const float* prec, const float* item_emb, const int64_t* excl_ptr, const int32_t* excl_idx,
                                   const uint8_t* cand, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K) {
    if (!topk_args_ok({prec, item_emb, excl_ptr, excl_idx, ids, scores}, prec, item_emb, ws, U, N1, E, K) ||
        (reinterpret_cast<uintptr_t>(excl_ptr) & 7u) != 0)
        return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t* w = static_cast<uint64_t*>(ws);
    return cand ? topk_excl_launch<true>(s, prec, item_emb, excl_ptr, excl_idx, cand, ids, scores, w, U, N1, E, K)
                : topk_excl_launch<false>(s, prec, item_emb, excl_ptr, excl_idx, nullptr, ids, scores, w, U, N1, E, K);
}

extern "C" int a4r_row_inv_norms(void* stream, const float* table, float* inv, int N1, int E) {
    if (!table || !inv || N1 < 1 || !width_served(WidthsF32{}, E) || !aligned16(table, nullptr)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    with_width(WidthsF32{}, E, [&](auto e) {
        hipLaunchKernelGGL(row_inv_norms_kernel<decltype(e)::value>, dim3((N1 + 15) / 16), dim3(256), 0, s, table, inv, N1);
    });
    return a4r_launch_status();
}

extern "C" int a4r_topk_similar(void* stream, const float* item_emb, const float* inv_norm, const int32_t* query, const uint8_t* cand,
                                float min_sim, int32_t* ids, float* scores, void* ws, int Q, int N1, int E, int K) {
    if (!topk_args_ok({item_emb, query, ids, scores}, item_emb, nullptr, ws, Q, N1, E, K) || min_sim != min_sim) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t* w = static_cast<uint64_t*>(ws);
    const auto launch = cand ? (inv_norm ? similar_launch<true, true> : similar_launch<true, false>)
                             : (inv_norm ? similar_launch<false, true> : similar_launch<false, false>);
    return launch(s, item_emb, inv_norm, query, cand, min_sim, ids, scores, w, Q, N1, E, K);
}

extern "C" size_t a4r_topk_ws_bytes(int U, int N1, int K) {
    if (!topk_shape_ok(U, N1, K)) return 0;
    return (size_t)topk_ranges(U, N1) * (size_t)U * (size_t)K * sizeof(uint64_t);
}

extern "C" size_t a4r_topk_bf16_ws_bytes(int U, int N1, int E, int K) {
    if (!topk_shape_ok(U, N1, K) || !width_served(WidthsF32{}, E)) return 0;
    return (size_t)topk_ranges(U, N1, topk_bf16_rs(E, K)) * (size_t)U * (size_t)K * sizeof(uint64_t);
}

extern "C" int a4r_topk_items_bf16(void* stream, const void* prec_b, const void* table_b, const int32_t* excl_ptr, const int32_t* excl_idx,
                                   const uint8_t* cand, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K) {
    if (!topk_args_ok({prec_b, table_b, excl_ptr, excl_idx, ids, scores}, prec_b, table_b, ws, U, N1, E, K)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    uint64_t* w = static_cast<uint64_t*>(ws);
    return cand ? topk_bf16_launch<true>(s, prec, table, excl_ptr, excl_idx, cand, ids, scores, w, U, N1, E, K)
                : topk_bf16_launch<false>(s, prec, table, excl_ptr, excl_idx, nullptr, ids, scores, w, U, N1, E, K);
}

extern "C" int a4r_topk_items(void* stream, const float* prec, const float* item_emb, const int32_t* excl_ptr, const int32_t* excl_idx,
                              int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K) {
    return topk_launch<false>(stream, prec, item_emb, excl_ptr, excl_idx, nullptr, ids, scores, ws, U, N1, E, K);
}

extern "C" int a4r_topk_items_cand(void* stream, const float* prec, const float* item_emb, const int32_t* excl_ptr, const int32_t* excl_idx,
                                   const uint8_t* cand, int32_t* ids, float* scores, void* ws, int U, int N1, int E, int K) {
    return topk_launch<true>(stream, prec, item_emb, excl_ptr, excl_idx, cand, ids, scores, ws, U, N1, E, K);
}
