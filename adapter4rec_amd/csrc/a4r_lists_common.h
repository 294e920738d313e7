// What the kernels that score a user's own rows share (a4r_lists.hip: the rows of a list the caller brings; a4r_eval_negatives.hip: the rows a
// sampled evaluation draws): the fixed-order gather-and-dot that makes score(u, i) a pure function of (u, i), the padded key buffer and its
// bitonic sort in LDS.  One definition, so the two files cannot drift apart: a sampled evaluation replays bit for bit through the list kernels.
#pragma once
#include "a4r_score_sweep.h"
#include "a4r_select.h"
#include "../../include/a4r.h"

namespace {

constexpr int MAXX = A4R_EVAL_MAX_HISTORY;   // exclusion / history ids per user kept in LDS
constexpr int XPER = (MAXX + 255) / 256;     // of them per thread while sorting

// a lane's part of <prec[u], row>: its V chunks in sequence, then the butterfly over the 16 lanes of the group (every lane ends with the sum)
template <int V> __device__ __forceinline__ float group_dot(const float4 (&p)[V], const float4 (&r)[V]) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < V; ++c) {
        acc = fmaf(p[c].x, r[c].x, acc);
        acc = fmaf(p[c].y, r[c].y, acc);
        acc = fmaf(p[c].z, r[c].z, acc);
        acc = fmaf(p[c].w, r[c].w, acc);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return acc;
}

template <int V> __device__ __forceinline__ void row_load(float4 (&r)[V], const float* __restrict__ table, int row, bool ok, int l16) {
#pragma unroll
    for (int c = 0; c < V; ++c)
        r[c] = ok ? *reinterpret_cast<const float4*>(table + (size_t)row * (V * 64) + (c * 16 + l16) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// keys[] is padded by one slot per 16 keys: a thread that owns 16 neighbouring keys (the last pass of every merge below) then starts 136 bytes
// from its neighbour, which spreads the 32 lanes of an 8-byte access over all 64 banks; unpadded they would meet on two.
__host__ __device__ __forceinline__ int kslot(int i) { return i + (i >> 4); }

// R = 2^RL keys per thread through RL steps of the bitonic network at once: the steps with strides J, J/2, ..., s = J >> (RL - 1) of merge length k
// touch, for a given key, only keys that differ from it in those RL index bits, so a thread that holds all 2^RL of them runs the steps in
// registers -- one LDS round trip and one barrier instead of RL.  The direction bit k lies above every stride of the pass: one direction per thread.
template <int RL> __device__ __forceinline__ void bitonic_pass(uint64_t* keys, int cap, int k, int J, int tid) {
    constexpr int R = 1 << RL;
    const int ls = __builtin_ctz(J) - (RL - 1), s = 1 << ls;
    for (int t = tid; t < (cap >> RL); t += 256) {
        const int base = ((t >> ls) << (ls + RL)) + (t & (s - 1));
        const bool desc = (base & k) == 0;
        uint64_t v[R];
#pragma unroll
        for (int m = 0; m < R; ++m) v[m] = keys[kslot(base + (m << ls))];
#pragma unroll
        for (int q = RL - 1; q >= 0; --q)
#pragma unroll
            for (int m = 0; m < R; ++m)
                if (!(m & (1 << q))) {
                    const uint64_t x = v[m], y = v[m | (1 << q)];
                    const bool sw = desc ? x < y : x > y;
                    v[m] = sw ? y : x;
                    v[m | (1 << q)] = sw ? x : y;
                }
#pragma unroll
        for (int m = 0; m < R; ++m) keys[kslot(base + (m << ls))] = v[m];
    }
}

// keys[0 .. cap) descending, cap a power of two >= 64.  A merge of length k has log2 k steps; they run RL at a time, RL as large as leaves every
// thread a group of keys (cap / 2^RL >= 256) and at most 4: 24 passes instead of 78 steps at cap = 4096, the plain network at cap <= 512.
__device__ __forceinline__ void bitonic_sort_desc(uint64_t* keys, int cap, int tid) {
    const int lc = __builtin_ctz(cap), rmax = lc <= 9 ? 1 : lc >= 12 ? 4 : lc - 8;
    for (int k = 2; k <= cap; k <<= 1)
        for (int rem = __builtin_ctz(k), J = k >> 1; rem > 0;) {
            const int r = rem < rmax ? rem : rmax;
            if (r == 1) bitonic_pass<1>(keys, cap, k, J, tid);
            else if (r == 2) bitonic_pass<2>(keys, cap, k, J, tid);
            else if (r == 3) bitonic_pass<3>(keys, cap, k, J, tid);
            else bitonic_pass<4>(keys, cap, k, J, tid);
            __syncthreads();
            J >>= r;
            rem -= r;
        }
}

__device__ __forceinline__ bool is_item(int id, int N1) { return (unsigned)id - 1u < (unsigned)(N1 - 1); }      // 1 <= id < N1

int lists_cap(int max_len) {                         // keys in LDS: the smallest power of two >= max(64, max_len)
    int c = 64;
    while (c < max_len) c <<= 1;
    return c;
}

}  // namespace
