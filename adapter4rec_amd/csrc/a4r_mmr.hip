// Diversified re-ranking of a top-K list by maximal marginal relevance (include/a4r_diversify.h states the rule): K greedy rounds over a pool of
// P <= 256 entries per user, each round an argmax of lambda * relevance - (1 - lambda) * (largest cosine to a selected entry) and an update of
// that largest cosine by the new pick.  The eager form gathers [U, P, E], forms the [U, P, P] Gram matrix and loops K times from the host; here
// nothing of that size exists: the K - 1 similarity updates are (K - 1) * P dot products per user, fewer than the Gram matrix's P * P.
//
// One 256-thread workgroup per user (grid-stride over users), thread j owns pool entry j: its id, score, norm, relevance r, largest cosine m,
// the running sum of 1 - c to the picks so far, and whether it is still to be had.
//   Set-up.  An entry is alive iff its id is an item and its score finite; alive[] in LDS holds the id, or 0.  Sixteen lanes own one row
//   (row_load / group_dot of a4r_lists_common.h: the fixed fma order and butterfly of the list kernels), 16 rows side by side, RF of them
//   requested per group before the first is used: <e_j, e_j> for every alive entry, once.  smin / smax by a wave butterfly and four LDS slots.
//   Round t.  key = orderable(v) << 32 | ~j, 0 for an entry that is not to be had: the maximum over the workgroup (wave butterfly, four LDS
//   slots) is the pick, the tie rule -- the smaller pool position -- inside the compare.  The owner of the pick writes ids / scores [t], adds its
//   sum of 1 - c to the user's total (one writer per round, in round order: the same bits every call) and leaves alive[].  Then every group loads
//   the pick's row and the rows of the alive entries are dotted with it, as above; thread j turns its dot into c, m = max(m, c), sum += 1 - c.
//   The last round ends at the pick.  No valid entry left: the remaining slots are id 0 / -inf.
//   ild = total / pairs: a pick's cosines to the picks before it were all formed while it was waiting.
// The pool's rows are re-read from L2 every round (P * E * 4 bytes: 25 KB .. 512 KB a user, read by this workgroup alone): one path for the four
// widths.  LDS: 2.1 KB.  No atomics, no scratch, no workspace.
#include "a4r_lists_common.h"   // group_dot, row_load, is_item

namespace {

__device__ __forceinline__ uint64_t mmr_key(float v, int j) {
    v += 0.f;                                        // -0 -> +0: one key
    const uint32_t b = __float_as_uint(v);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);      // monotone in v (v is never NaN: r and m are finite)
    return ((uint64_t)o << 32) | (uint32_t)~(uint32_t)j;               // j <= 255: the low half is never 0, so no live key is 0
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// s_dot[j] = <sel, item_emb[alive[j]]> for every j < P with alive[j] != 0 (0 for the others); SELF: <row, row> instead, sel unused
template <int V, bool SELF>
__device__ __forceinline__ void pool_dots(const float* __restrict__ item_emb, const float4 (&sel)[V], const int32_t* alive, float* s_dot, int P,
                                          int g, int l16) {
    constexpr int RF = V >= 4 ? 2 : 8 / V;           // rows a group requests before it uses the first (lists_kernel's)
    for (int base = 0; base < P; base += 16 * RF) {
        float4 rw[RF][V];
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int j = base + r * 16 + g;
            const int id = j < P ? alive[j] : 0;
            row_load<V>(rw[r], item_emb, id, id != 0, l16);
        }
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int j = base + r * 16 + g;
            const float d = SELF ? group_dot<V>(rw[r], rw[r]) : group_dot<V>(sel, rw[r]);
            if (l16 == 0 && j < P) s_dot[j] = d;
        }
    }
}

template <int E>
__global__ void __launch_bounds__(256) mmr_kernel(const float* __restrict__ item_emb, const int32_t* __restrict__ pool_ids,
                                                  const float* __restrict__ pool_scores, int32_t* __restrict__ ids, float* __restrict__ scores,
                                                  float* __restrict__ ild, float lambda, int U, int N1, int P, int K) {
    constexpr int V = E / 64;                        // 16-byte chunks of a row per lane
    __shared__ int32_t alive[256];                   // the entry's id while it is valid and unselected, else 0
    __shared__ float s_dot[256];
    __shared__ uint64_t s_key[4];
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int32_t s_pick_id;
    __shared__ float s_pick_norm, s_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = tid & 15, g = tid >> 4;
    const float oml = 1.f - lambda, inf = __builtin_huge_valf();
    for (int u = blockIdx.x; u < U; u += gridDim.x) {
        int pid = 0;
        float ps = 0.f;
        if (tid < P) {
            pid = pool_ids[(size_t)u * P + tid];
            ps = pool_scores[(size_t)u * P + tid];
        }
        bool live = tid < P && is_item(pid, N1) && fabsf(ps) < inf;         // (NaN compares false)
        alive[tid] = live ? pid : 0;
        float lo = live ? ps : inf, hi = live ? ps : -inf;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
        if (tid == 0) s_total = 0.f;
        __syncthreads();
        float4 sel[V];
        pool_dots<V, true>(item_emb, sel, alive, s_dot, P, g, l16);
        lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
        __syncthreads();
        const float nrm = live ? sqrtf(s_dot[tid]) : 0.f;
        const float r = !live ? 0.f : hi == lo ? 1.f : (float)(((double)ps - (double)lo) / ((double)hi - (double)lo));
        float m = -inf, dsum = 0.f;                  // m: the largest cosine to a pick, once there is one (a cosine may be negative)
        int32_t* oi = ids + (size_t)u * K;
        float* os = scores + (size_t)u * K;
        int n = 0;                                   // picks so far (uniform)
        while (n < K) {
            const float v = fmaf(lambda, r, -(oml * (n == 0 ? 0.f : m)));
            uint64_t key = wave_max_u64(live ? mmr_key(v, tid) : 0ull);
            if (lane == 0) s_key[wave] = key;
            __syncthreads();                         // (also: the s_dot of the round before is read by now)
            key = s_key[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
            if (key == 0) break;                     // (uniform) no valid entry left
            const int js = (int)~(uint32_t)key;
            if (tid == js) {
                oi[n] = pid;
                os[n] = ps;
                s_total += dsum;
                s_pick_id = pid;
                s_pick_norm = nrm;
                alive[tid] = 0;
                live = false;
            }
            ++n;
            if (n == K) break;                       // the last pick updates nothing
            __syncthreads();
            row_load<V>(sel, item_emb, s_pick_id, true, l16);
            pool_dots<V, false>(item_emb, sel, alive, s_dot, P, g, l16);
            __syncthreads();
            if (live) {
                const float pn = s_pick_norm;
                const float c = (pn == 0.f || nrm == 0.f) ? 0.f : s_dot[tid] / (pn * nrm);
                m = fmaxf(m, c);
                dsum += 1.f - c;
            }
        }
        for (int j = n + tid; j < K; j += 256) { oi[j] = 0; os[j] = -inf; }
        __syncthreads();
        if (tid == 0 && ild) ild[u] = n >= 2 ? s_total / (float)(n * (n - 1) / 2) : 0.f;
        __syncthreads();                             // the next user overwrites alive, s_total and the slots
    }
}

}  // namespace

extern "C" int a4r_mmr_rerank(void* stream, const float* item_emb, const int32_t* pool_ids, const float* pool_scores, int32_t* ids, float* scores,
                              float* ild, float lambda, int U, int N1, int E, int P, int K) {
    if (!item_emb || !pool_ids || !pool_scores || !ids || !scores) return A4R_EINVAL;
    if (U < 1 || N1 < 2 || !width_served(WidthsF32{}, E) || P < 1 || P > A4R_MMR_MAX_POOL || K < 1 || K > P) return A4R_EINVAL;
    if (!(lambda >= 0.f && lambda <= 1.f) || !aligned16(item_emb, nullptr)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = U < 65536 ? U : 65536;          // one workgroup per user; past that they stride
    with_width(WidthsF32{}, E, [&](auto e) {
        hipLaunchKernelGGL((mmr_kernel<decltype(e)::value>), dim3(grid), dim3(256), 0, s, item_emb, pool_ids, pool_scores, ids, scores, ild, lambda, U,
                           N1, P, K);
    });
    return a4r_launch_status();
}
