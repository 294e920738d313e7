// Top-K and rank within a candidate list of each user's own (include/a4r_user_lists.h): the shortlist of a retrieval stage, or the negatives of a
// sampled evaluation.  Not a table sweep: every user reads other rows, a few hundred to a few thousand of them, so this is a batched GEMV whose
// cost is the gather of 256 B .. 2 KB rows -- the MFMA kernels of a4r_topk.hip / a4r_eval.hip, which share one table tile among 16 users, have
// nothing to share here.
//
// One 256-thread workgroup per user (grid-stride over users).
//   Set-up.  The user's exclusion / history ids are copied to LDS and put in ascending order (rank_sort_i32 of a4r_select.h); every lane
//   keeps its E / 16 floats of the user's prec row in registers.
//   Gather and score.  Sixteen lanes own one listed row: lane l reads the 16-byte chunks l, l + 16, ... of the row (one 256-byte line per load
//   of the group), multiplies them into its own accumulator in sequence (fma), and the 16 accumulators meet in a four-step xor butterfly --
//   a fixed order that depends on E alone, so score(u, i) has the same bits wherever i stands in whichever list.  A group requests RF rows
//   (8 .. 16 loads of 16 bytes per lane) before it uses the first, and the ids of the next RF rows before that: the loop waits on memory, not
//   on arithmetic.  A row whose id is no item (0, negative, >= N1) is not requested at all.
//   Keys.  Lane r of the group takes the r-th of its RF rows (every lane holds every sum): it searches the exclusion list and writes the row's
//   64-bit key (a4r_select.h), or 0, to keys[j] in LDS, j = the row's place in the list -- RF searches side by side, not one after the other.  The tail up to the next power of two (at least 64) is zeroed and the keys are sorted descending, bitonic, in LDS,
//   up to four steps of the network per LDS round trip (bitonic_pass).
//   An id listed twice gave the same key twice (the score is a pure function), and equal keys are now adjacent: a key is kept if it is not 0
//   and differs from its left neighbour.
//   Top-K.  The kept keys are numbered by ballot and wave totals, 256 positions a round, and the first K decoded to ids / scores; the rounds end
//   when K are out or the keys are.  No second sort.
//   Rank.  The target's score comes from the same instruction sequence; the kept keys whose score half exceeds the target's are counted and
//   summed over the workgroup.
// LDS: the keys (8 bytes x 17/16 of the power of two above max_len: 34 KiB at A4R_LIST_MAX) + 1.1 KB.  No atomics, no scratch, no workspace.
#include "a4r_lists_common.h"   // group_dot, row_load, kslot, the bitonic sort, is_item, lists_cap: shared with a4r_eval_negatives.hip

namespace {

// RANK = false: ids / scores [U, K] (target, rank unused).  RANK = true: rank [U] (ids, scores, K unused); x_* is then the history.
template <int E, bool RANK>
__global__ void __launch_bounds__(256) lists_kernel(const float* __restrict__ prec, const float* __restrict__ item_emb,
                                                    const int32_t* __restrict__ target, const int32_t* __restrict__ list_ptr,
                                                    const int32_t* __restrict__ list_idx, const int32_t* __restrict__ x_ptr,
                                                    const int32_t* __restrict__ x_idx, int32_t* __restrict__ ids, float* __restrict__ scores,
                                                    int32_t* __restrict__ rank, int U, int N1, int K, int max_len) {
    constexpr int V = E / 64;                        // 16-byte chunks of a row per lane
    constexpr int RF = V >= 4 ? 2 : 8 / V;           // rows a group requests before it uses the first: 8, 4, 2, 2 -> 8, 8, 8, 16 loads in flight per lane
    extern __shared__ uint64_t keys[];               // [cap + cap / 16]: kslot
    __shared__ int32_t excl[MAXX];
    __shared__ int32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = tid & 15, g = tid >> 4;
    for (int u = blockIdx.x; u < U; u += gridDim.x) {
        const int xb = x_ptr[u], nx = max(0, min(x_ptr[u + 1] - xb, MAXX));
        for (int j = tid; j < nx; j += 256) excl[j] = x_idx[xb + j];
        float4 p[V];
        row_load<V>(p, prec, u, true, l16);
        const int lb = list_ptr[u], n = max(0, min(list_ptr[u + 1] - lb, max_len));
        int idn[RF];                                 // the ids of the group's next RF rows
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int j = r * 16 + g;
            idn[r] = j < n ? list_idx[lb + j] : 0;
        }
        int cap = 64;                                // this user's sort length
        while (cap < n) cap <<= 1;
        for (int j = n + tid; j < cap; j += 256) keys[kslot(j)] = 0;
        [[maybe_unused]] uint32_t thi = 0xffffffffu;   // RANK: the target's score half (no item: nothing beats it)
        if constexpr (RANK) {
            const int t = target[u];
            if (is_item(t, N1)) {                    // (uniform: every group forms the target's score, by the sequence every listed row goes through)
                float4 rw[V];
                row_load<V>(rw, item_emb, t, true, l16);
                thi = (uint32_t)(topk_key(group_dot<V>(p, rw), 0) >> 32);
            }
        }
        __syncthreads();
        rank_sort_i32<XPER, 256>(excl, nx, tid);     // the exclusion ids in ascending order
        __syncthreads();
        for (int base = 0; base < n; base += 16 * RF) {
            int id[RF];
            bool ok[RF];
            float4 rw[RF][V];
#pragma unroll
            for (int r = 0; r < RF; ++r) {
                id[r] = idn[r];
                ok[r] = is_item(id[r], N1);
                row_load<V>(rw[r], item_emb, id[r], ok[r], l16);
            }
#pragma unroll
            for (int r = 0; r < RF; ++r) {
                const int j = base + 16 * RF + r * 16 + g;
                idn[r] = j < n ? list_idx[lb + j] : 0;
            }
            // every lane of the group ends with every row's sum and id: lane r takes row r, so the RF searches of the group run side by side
            int my_id = 0;
            float my_s = 0.f;
            bool my_ok = false;
#pragma unroll
            for (int r = 0; r < RF; ++r) {
                const float s = group_dot<V>(p, rw[r]);
                if (l16 == r) { my_id = id[r]; my_s = s; my_ok = ok[r]; }
            }
            const int j = base + l16 * 16 + g;
            if (l16 < RF && j < n) {
                uint64_t key = 0;
                if (my_ok && !sorted_has(excl, nx, my_id)) key = topk_key(my_s, my_id);
                keys[kslot(j)] = key;
            }
        }
        __syncthreads();
        bitonic_sort_desc(keys, cap, tid);
        if constexpr (RANK) {
            int c = 0;
            for (int i = tid; i < cap; i += 256) {
                const uint64_t x = keys[kslot(i)];
                c += (x != 0 && (i == 0 || keys[kslot(i - 1)] != x) && (uint32_t)(x >> 32) > thi) ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) wsum[wave] = c;
            __syncthreads();
            if (tid == 0) rank[u] = 1 + wsum[0] + wsum[1] + wsum[2] + wsum[3];
        } else {
            int32_t* oi = ids + (size_t)u * K;
            float* os = scores + (size_t)u * K;
            int done = 0;                            // kept keys of the rounds before
            for (int r0 = 0; r0 < cap && done < K && keys[kslot(r0)] != 0; r0 += 256) {      // (uniform; the keys past the first 0 are all 0)
                const int i = r0 + tid;
                const uint64_t x = i < cap ? keys[kslot(i)] : 0;
                const bool kept = x != 0 && (i == 0 || keys[kslot(i - 1)] != x);
                const uint64_t bal = __ballot(kept);
                if (lane == 0) wsum[wave] = __popcll(bal);
                __syncthreads();
                int at = done + __popcll(bal & ((1ull << lane) - 1ull));
                for (int w = 0; w < wave; ++w) at += wsum[w];
                if (kept && at < K) topk_emit(x, oi + at, os + at);
                done += wsum[0] + wsum[1] + wsum[2] + wsum[3];
                __syncthreads();
            }
            for (int j = done + tid; j < K; j += 256) topk_emit(0, oi + j, os + j);
        }
        __syncthreads();                             // the next user overwrites excl, keys and wsum
    }
}

bool lists_shape_ok(int U, int N1, int E, int max_len, const float* prec, const float* item_emb) {
    return U >= 1 && N1 >= 2 && width_served(WidthsF32{}, E) && max_len >= 0 && max_len <= A4R_LIST_MAX && aligned16(prec, item_emb);
}

template <bool RANK>
int lists_launch(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* list_ptr, const int32_t* list_idx,
                 const int32_t* x_ptr, const int32_t* x_idx, int32_t* ids, float* scores, int32_t* rank, int U, int N1, int E, int K, int max_len) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = (size_t)kslot(lists_cap(max_len)) * sizeof(uint64_t);
    const int grid = U < 65536 ? U : 65536;          // one workgroup per user; past that they stride
    with_width(WidthsF32{}, E, [&](auto e) {
        hipLaunchKernelGGL((lists_kernel<decltype(e)::value, RANK>), dim3(grid), dim3(256), lds, s, prec, item_emb, target, list_ptr, list_idx, x_ptr,
                           x_idx, ids, scores, rank, U, N1, K, max_len);
    });
    return a4r_launch_status();
}

}  // namespace

extern "C" int a4r_topk_lists(void* stream, const float* prec, const float* item_emb, const int32_t* list_ptr, const int32_t* list_idx,
                              const int32_t* excl_ptr, const int32_t* excl_idx, int32_t* ids, float* scores, int U, int N1, int E, int K,
                              int max_len) {
    if (!prec || !item_emb || !list_ptr || !list_idx || !excl_ptr || !excl_idx || !ids || !scores) return A4R_EINVAL;
    if (!lists_shape_ok(U, N1, E, max_len, prec, item_emb) || K < 1 || K > A4R_TOPK_MAX_K) return A4R_EINVAL;
    return lists_launch<false>(stream, prec, item_emb, nullptr, list_ptr, list_idx, excl_ptr, excl_idx, ids, scores, nullptr, U, N1, E, K, max_len);
}

extern "C" int a4r_eval_rank_lists(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* list_ptr,
                                   const int32_t* list_idx, const int32_t* hist_ptr, const int32_t* hist_idx, int32_t* rank, int U, int N1, int E,
                                   int max_len) {
    if (!prec || !item_emb || !target || !list_ptr || !list_idx || !hist_ptr || !hist_idx || !rank) return A4R_EINVAL;
    if (!lists_shape_ok(U, N1, E, max_len, prec, item_emb)) return A4R_EINVAL;
    return lists_launch<true>(stream, prec, item_emb, target, list_ptr, list_idx, hist_ptr, hist_idx, nullptr, nullptr, rank, U, N1, E, 0, max_len);
}
