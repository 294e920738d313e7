// What the selection kernels share (a4r_topk.hip over the item table, a4r_lists.hip over a user's own list, a4r_eval_negatives.hip over drawn rows):
// the 64-bit selection key and its decoding, and the sorting and searching of a user's id list (exclusions, history) in LDS.
//   key = orderable(score) << 32 | ~id : one unsigned compare orders by score descending, then id ascending; NaN maps below -inf, -0 onto +0;
//   key 0 is "no item".  The upper half alone orders by score (what a rank compares).
#pragma once
#include "a4r_common.h"

namespace {

__device__ __forceinline__ uint64_t topk_key(float s, int id) {
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;                                           // -0 == +0: one key
    uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);              // monotone in the float value
    if (s != s) o = 0u;                                                     // NaN: below -inf
    return ((uint64_t)o << 32) | (uint32_t)~(uint32_t)id;
}

__device__ __forceinline__ void topk_emit(uint64_t key, int32_t* id, float* score) {
    if (key == 0) { *id = 0; *score = -__builtin_huge_valf(); return; }    // short list: pad slot
    const uint32_t o = (uint32_t)(key >> 32);
    *id = (int32_t)~(uint32_t)key;
    *score = o == 0 ? __builtin_nanf("") : __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// list[0 .. n) in LDS into ascending order, in place.  STRIDE threads own a list, thread j0 = 0 .. STRIDE - 1 of them the ids j0, j0 + STRIDE, ...
// (PER each: n <= PER * STRIDE); every thread of the workgroup calls it, behind the barrier that follows the list's last store.  An id goes to
// its rank: the number of ids that are smaller, or equal and in front of it -- ties by position, which makes the ranks a permutation: every slot
// is written once.  The barrier stands between the last read of the unsorted list and the first write; the one before the first search is the
// caller's.
template <int PER, int STRIDE> __device__ __forceinline__ void rank_sort_i32(int32_t* list, int n, int j0) {
    int v[PER], pos[PER];
#pragma unroll
    for (int m = 0; m < PER; ++m) {
        const int j = j0 + STRIDE * m;
        pos[m] = -1; v[m] = 0;
        if (j < n) {
            const int x = list[j];
            int p = 0;
            for (int k = 0; k < n; ++k) {
                const int y = list[k];
                p += (y < x || (y == x && k < j)) ? 1 : 0;
            }
            v[m] = x; pos[m] = p;
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < PER; ++m)
        if (pos[m] >= 0) list[pos[m]] = v[m];
}

// is id in list[0 .. n), ascending?  (the first position holding an id >= id, then one compare)
__device__ __forceinline__ bool sorted_has(const int32_t* list, int n, int id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && list[lo] == id;
}

}  // namespace
