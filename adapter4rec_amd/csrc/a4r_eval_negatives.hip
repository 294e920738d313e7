// The negatives of a sampled evaluation drawn on the device (include/a4r_eval_negatives.h): a4r_eval_draw_negatives materialises them,
// a4r_eval_rank_sampled draws, gathers, scores and ranks in one launch -- no [U, N] id matrix, no CSR, no second launch.
//
// One 256-thread workgroup per user (grid-stride over users), as lists_kernel of a4r_lists.hip, whose scoring and sort this file shares through
// a4r_lists_common.h.
//   Set-up (draw_setup).  The user's history ids and the target go into LDS (ids that are no item as 0), are put in ascending order by rank
//   counting, and the first of every run of equal non-zero ids is kept: D, at most 265 ids, numbered by ballot and wave totals.  Beside D[k] stand
//   P[k] = the mass of D[0 .. k) and G[k] = cdf[D[k] - 1] - P[k], the draw value from which on the walk of the rule steps over D[k].  G is
//   non-decreasing (G[k + 1] - G[k] = cdf[D[k + 1] - 1] - cdf[D[k]] >= 0) and the walk steps over a prefix of D, so
//       x_final = x + P[c],  c = #{k : G[k] <= x}     -- one binary search over <= 265 int64 in LDS instead of 265 dependent steps.
//   Uniform sampling (cdf == NULL) is cnt = 1: P[k] = k, G[k] = D[k] - 1 - k, no global read at all.
//   Draw.  Thread t draws j = t, t + 256, ...: the counter hash, a 64 x 64 high product, the search in LDS and, under popularity sampling, a
//   binary search of cdf (log2 N1 dependent 8-byte vector loads of an L2-resident array).
//   Rank.  The drawn ids are parked in the low words of the key slots they will occupy: the 16 lanes that own row j read slot j one round before
//   lane r of the same group -- the same wave, in program order -- overwrites it with the row's key, so the ids need no LDS of their own.  From
//   there on this is lists_kernel<E, true>: RF rows requested before the first is used, group_dot, keys, bitonic sort, kept keys above the
//   target's score half counted.  The search of the history is left out: a drawn id is never in D.
// LDS: the keys (8 bytes x 17/16 of the power of two above N: 34 KiB at A4R_LIST_MAX) + 6.4 KB of set-up.  The one atomic is the integer add on *err.
#include "a4r_lists_common.h"

namespace {

constexpr int MAXD = MAXX + 1;               // the history and the target
constexpr int DPER = (MAXD + 255) / 256;     // of them per thread while sorting
constexpr int PPER = (MAXD + 1 + 255) / 256; // prefix masses P[0 .. d] per thread

struct DrawLds {
    int32_t raw[MAXD];                       // history + target, then the same in ascending order
    int32_t dset[MAXD];                      // D: distinct items ascending
    int64_t G[MAXD];                         // cdf[D[k] - 1] - P[k]
    int64_t P[MAXD + 1];                     // mass of D[0 .. k); P[d] = the mass of D
    int32_t wsum[4];
};

__device__ __forceinline__ int64_t cdf_at(const int64_t* __restrict__ cdf, int i) { return cdf ? cdf[i] : (int64_t)i; }

// every thread of the workgroup calls it; -> (d = |D|, m); L is ready for draw_one when it returns
__device__ __forceinline__ void draw_setup(DrawLds& L, const int32_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int t,
                                           const int64_t* __restrict__ cdf, int u, int N1, int tid, int& d_out, int64_t& m_out) {
    const int lane = tid & 63, wave = tid >> 6;
    const int xb = hist_ptr[u], nx = max(0, min(hist_ptr[u + 1] - xb, MAXX)), n = nx + 1;
    for (int j = tid; j < nx; j += 256) {
        const int x = hist_idx[xb + j];
        L.raw[j] = is_item(x, N1) ? x : 0;
    }
    if (tid == 0) L.raw[nx] = is_item(t, N1) ? t : 0;
    __syncthreads();
    rank_sort_i32<DPER, 256>(L.raw, n, tid);
    __syncthreads();
    int d = 0;                                       // the first of every run of equal non-zero ids, numbered in order
#pragma unroll
    for (int q = 0; q < DPER; ++q) {
        const int i = tid + 256 * q;
        const int v = i < n ? L.raw[i] : 0;
        const bool keep = v != 0 && (i == 0 || L.raw[i - 1] != v);
        const uint64_t bal = __ballot(keep);
        if (lane == 0) L.wsum[wave] = __popcll(bal);
        __syncthreads();
        int at = d + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) at += L.wsum[w];
        if (keep) {
            L.dset[at] = v;
            L.P[at + 1] = cdf_at(cdf, v) - cdf_at(cdf, v - 1);       // cnt[v], summed below
        }
        d += L.wsum[0] + L.wsum[1] + L.wsum[2] + L.wsum[3];
        __syncthreads();
    }
    {   // P[k] = cnt[D[0]] + ... + cnt[D[k - 1]], k = 0 .. d: every thread sums its own prefix (LDS broadcasts), then all write
        int64_t s[PPER];
#pragma unroll
        for (int q = 0; q < PPER; ++q) {
            const int k = tid + 256 * q;
            s[q] = 0;
            if (k <= d)
                for (int i = 1; i <= k; ++i) s[q] += L.P[i];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPER; ++q) {
            const int k = tid + 256 * q;
            if (k <= d) L.P[k] = s[q];
            if (k < d) L.G[k] = cdf_at(cdf, L.dset[k] - 1) - s[q];
        }
    }
    __syncthreads();
    d_out = d;
    m_out = cdf_at(cdf, N1 - 1) - L.P[d];
}

// draw j of the user with key uk; m >= 1
__device__ __forceinline__ int draw_one(const DrawLds& L, const int64_t* __restrict__ cdf, uint64_t seed, int uk, int j, int d, int64_t m, int N1) {
    const uint64_t h = a4r_hash64(seed, A4R_EVAL_NEG_SITE, ((uint64_t)(uint32_t)uk << 16) | (uint64_t)j);
    const int64_t x0 = (int64_t)__umul64hi(h, (uint64_t)m);           // uniform over 0 .. m-1
    int lo = 0, hi = d;                                                // c = #{k : G[k] <= x0}
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (L.G[mid] <= x0) lo = mid + 1; else hi = mid;
    }
    const int64_t x = x0 + L.P[lo];                                    // < cdf[N1 - 1]
    if (!cdf) return (int)(x + 1);
    int a = 1, b = N1 - 1;                                             // the smallest i with cdf[i] > x
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (cdf[mid] > x) b = mid; else a = mid + 1;
    }
    return a;
}

__global__ void __launch_bounds__(256) draw_kernel(const int32_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx,
                                                   const int32_t* __restrict__ target, const int32_t* __restrict__ user_key,
                                                   const int64_t* __restrict__ cdf, uint64_t seed, int32_t* __restrict__ out_ids,
                                                   int32_t* __restrict__ err, int U, int N1, int N) {
    __shared__ DrawLds L;
    const int tid = threadIdx.x;
    for (int u = blockIdx.x; u < U; u += gridDim.x) {
        int d;
        int64_t m;
        draw_setup(L, hist_ptr, hist_idx, target[u], cdf, u, N1, tid, d, m);
        const int uk = user_key[u];
        if (m < 1 && tid == 0) atomicAdd(err, 1);
        int32_t* out = out_ids + (size_t)u * N;
        for (int j = tid; j < N; j += 256) out[j] = m < 1 ? 0 : draw_one(L, cdf, seed, uk, j, d, m, N1);
        __syncthreads();                             // the next user overwrites L
    }
}

template <int E>
__global__ void __launch_bounds__(256) rank_sampled_kernel(const float* __restrict__ prec, const float* __restrict__ item_emb,
                                                           const int32_t* __restrict__ target, const int32_t* __restrict__ hist_ptr,
                                                           const int32_t* __restrict__ hist_idx, const int32_t* __restrict__ user_key,
                                                           const int64_t* __restrict__ cdf, uint64_t seed, int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ err, int U, int N1, int N, int cap) {
    constexpr int V = E / 64;                        // 16-byte chunks of a row per lane
    constexpr int RF = V >= 4 ? 2 : 8 / V;           // rows a group requests before it uses the first (lists_kernel's)
    extern __shared__ uint64_t keys[];               // [cap + cap / 16]: kslot; cap = lists_cap(N)
    __shared__ DrawLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = tid & 15, g = tid >> 4;
    for (int u = blockIdx.x; u < U; u += gridDim.x) {
        float4 p[V];
        row_load<V>(p, prec, u, true, l16);
        const int t = target[u], uk = user_key[u];
        uint32_t thi = 0xffffffffu;                  // the target's score half (no item: nothing beats it)
        if (is_item(t, N1)) {                        // (uniform: every group forms the target's score, by the sequence every drawn row goes through)
            float4 rw[V];
            row_load<V>(rw, item_emb, t, true, l16);
            thi = (uint32_t)(topk_key(group_dot<V>(p, rw), 0) >> 32);
        }
        int d;
        int64_t m;
        draw_setup(L, hist_ptr, hist_idx, t, cdf, u, N1, tid, d, m);
        if (m < 1) {                                 // (uniform) no candidate: N draws of 0, rank 1, counted once
            if (tid == 0) {
                atomicAdd(err, 1);
                rank[u] = 1;
            }
            __syncthreads();
            continue;
        }
        for (int j = tid; j < cap; j += 256) keys[kslot(j)] = j < N ? (uint64_t)(uint32_t)draw_one(L, cdf, seed, uk, j, d, m, N1) : 0;
        __syncthreads();
        int idn[RF];                                 // the ids of the group's next RF rows
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int j = r * 16 + g;
            idn[r] = j < N ? (int)(uint32_t)keys[kslot(j)] : 0;
        }
        for (int base = 0; base < N; base += 16 * RF) {
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
            for (int r = 0; r < RF; ++r) {           // slots of the next round: this group's own, not yet overwritten (it writes them a round later)
                const int j = base + 16 * RF + r * 16 + g;
                idn[r] = j < N ? (int)(uint32_t)keys[kslot(j)] : 0;
            }
            int my_id = 0;
            float my_s = 0.f;
            bool my_ok = false;
#pragma unroll
            for (int r = 0; r < RF; ++r) {
                const float s = group_dot<V>(p, rw[r]);
                if (l16 == r) { my_id = id[r]; my_s = s; my_ok = ok[r]; }
            }
            const int j = base + l16 * 16 + g;
            if (l16 < RF && j < N) keys[kslot(j)] = my_ok ? topk_key(my_s, my_id) : 0;
        }
        __syncthreads();
        bitonic_sort_desc(keys, cap, tid);
        int c = 0;
        for (int i = tid; i < cap; i += 256) {
            const uint64_t x = keys[kslot(i)];
            c += (x != 0 && (i == 0 || keys[kslot(i - 1)] != x) && (uint32_t)(x >> 32) > thi) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) L.wsum[wave] = c;
        __syncthreads();
        if (tid == 0) rank[u] = 1 + L.wsum[0] + L.wsum[1] + L.wsum[2] + L.wsum[3];
        __syncthreads();                             // the next user overwrites L and keys
    }
}

bool draw_shape_ok(int U, int N1, int N) { return U >= 1 && N1 >= 2 && N >= 1 && N <= A4R_LIST_MAX; }

}  // namespace

extern "C" int a4r_eval_draw_negatives(void* stream, const int32_t* hist_ptr, const int32_t* hist_idx, const int32_t* target,
                                       const int32_t* user_key, const int64_t* cdf, uint64_t seed, int32_t* out_ids, int32_t* err, int U, int N1,
                                       int N) {
    if (!hist_ptr || !hist_idx || !target || !user_key || !out_ids || !err) return A4R_EINVAL;
    if (!draw_shape_ok(U, N1, N)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = U < 65536 ? U : 65536;          // one workgroup per user; past that they stride
    hipLaunchKernelGGL(draw_kernel, dim3(grid), dim3(256), 0, s, hist_ptr, hist_idx, target, user_key, cdf, seed, out_ids, err, U, N1, N);
    return a4r_launch_status();
}

extern "C" int a4r_eval_rank_sampled(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* hist_ptr,
                                     const int32_t* hist_idx, const int32_t* user_key, const int64_t* cdf, uint64_t seed, int32_t* rank,
                                     int32_t* err, int U, int N1, int E, int N) {
    if (!prec || !item_emb || !target || !hist_ptr || !hist_idx || !user_key || !rank || !err) return A4R_EINVAL;
    if (!draw_shape_ok(U, N1, N) || !width_served(WidthsF32{}, E) || !aligned16(prec, item_emb)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cap = lists_cap(N);
    const size_t lds = (size_t)kslot(cap) * sizeof(uint64_t);
    const int grid = U < 65536 ? U : 65536;
    with_width(WidthsF32{}, E, [&](auto e) {
        hipLaunchKernelGGL((rank_sampled_kernel<decltype(e)::value>), dim3(grid), dim3(256), lds, s, prec, item_emb, target, hist_ptr, hist_idx,
                           user_key, cdf, seed, rank, err, U, N1, N, cap);
    });
    return a4r_launch_status();
}
