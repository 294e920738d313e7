// The 64-bit selection key of the top-K kernels (a4r_topk.hip over the item table, a4r_lists.hip over a user's own list) and its decoding.
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

}  // namespace
