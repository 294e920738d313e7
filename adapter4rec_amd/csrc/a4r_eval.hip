// Eval: rank of the held-out target among all items (data_utils/metrics.py:82-116) without
// materialising the [users, items] score matrix and without the per-user Python loop.
//
// rank[u] = 1 + #{ i in [1, N1) : i not in hist(u), score(u, i) > score(u, target[u]) }.
// A workgroup owns 16 users and walks the table by the item-table score sweep (a4r_score_sweep.h),
// fp32, requested one tile ahead (the item table is read once per 16 users; it is L2/Infinity-Cache
// resident).  The target's score is produced by the very same instruction sequence (B rows = the
// 16 users' target items, diagonal taken), so the comparison is bit-consistent.  History items are excluded by counting every item first and taking back the user's
// (<= A4R_EVAL_MAX_HISTORY, distinct) history ids that beat the target -- their scores from the same instruction sequence again.  fp32 throughout: ranks are integers (bit-exact
// against the oracle up to fp32 summation order of the 64-term dot products).
#include "a4r_score_sweep.h"
#include "../../include/a4r.h"

namespace {

constexpr int MAXH = A4R_EVAL_MAX_HISTORY;   // history ids per user kept in LDS (reference keeps <= max_seq_len + 2 = 22; the engine allows max_seq_len <= 255)

// CAND (a4r_eval_rank_cand, include/a4r_candidates.h): only the items i with cand[i] != 0 are counted -- one byte per table row, read from global
// memory (cache-resident: 500 KB at 500 000 items), the byte of a wave's next tile requested with that tile's fragments.  CAND = false is the
// kernel as it was: every `if constexpr (CAND)` below drops out of it, and cand is never read.
template <int E, bool CAND>
__global__ void __launch_bounds__(256) eval_rank_kernel(const float* __restrict__ prec, const float* __restrict__ item_emb,
                                                        const int32_t* __restrict__ target, const int32_t* __restrict__ hist_ptr,
                                                        const int32_t* __restrict__ hist_idx, int32_t* __restrict__ rank, int U, int N1,
                                                        const uint8_t* __restrict__ cand) {
    constexpr int KS = E / 16;                       // chunk steps (fp32: 16 k per step)
    __shared__ int32_t hist[16][MAXH];
    __shared__ int32_t nhist[16];
    __shared__ float tscore[16];
    __shared__ int32_t cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * 16;
    {   // 16 threads per user copy its history ids
        const int ul = tid >> 4, u = min(u0 + ul, U - 1);
        const int b = hist_ptr[u], n = min(hist_ptr[u + 1] - b, MAXH);
        for (int j = tid & 15; j < n; j += 16) hist[ul][j] = hist_idx[b + j];
        if ((tid & 15) == 0) { nhist[ul] = n; cnt[ul] = 0; }
    }
    uint4 ua[KS];                                    // A operand: the 16 users
    const int urow = min(u0 + r16, U - 1);
    frag_load<E>(ua, prec, urow, kg);
    // target scores: B rows = target items of the 16 users, keep the diagonal
    {
        uint4 b[KS];
        frag_load<E>(b, item_emb, target[urow], kg);
        const f32x4_t acc = score_tile<float>(ua, b);
        // element (row = kg*4 + rr, col = r16): diagonal where kg*4 + rr == r16
        if (wave == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                if (kg * 4 + rr == r16) tscore[r16] = acc[rr];
        }
    }
    __syncthreads();
    float ts[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) ts[rr] = tscore[kg * 4 + rr];
    int local[4] = {0, 0, 0, 0};
    // The sweep itself -- the deal, the request one tile ahead and the score tile of a4r_score_sweep.h, as topk_partial_kernel runs them -- is
    // written out here: through SweepDeal / sweep_next / score_tile this loop gave the same bits but, the compiler scheduling it another
    // way, a launch 9 % slower at E = 128 (and 22 % faster at E = 64); piece by piece it ran up to twice as long (profiles/LOG.md).
    const int ntiles = (N1 - 1 + 15) / 16, tstep = gridDim.y * 4;
    int t = blockIdx.y * 4 + wave;
    uint4 bn[KS];
    [[maybe_unused]] uint8_t cn = 0;                 // CAND: the candidate byte of this lane's item in the requested tile
    {
        const int irow = min(1 + min(t, ntiles - 1) * 16 + r16, N1 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(item_emb + (size_t)irow * E + (ks * 4 + kg) * 4);
        if constexpr (CAND) cn = cand[irow];
    }
    for (; t < ntiles; t += tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column
        uint4 b[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = bn[ks];
        [[maybe_unused]] const uint8_t c = cn;
        {
            const int irow = min(1 + min(t + tstep, ntiles - 1) * 16 + r16, N1 - 1);      // (past the end: the last tile again, never used)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(item_emb + (size_t)irow * E + (ks * 4 + kg) * 4);
            if constexpr (CAND) cn = cand[irow];
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Mma<float>::mma(ua[ks], b[ks], acc);
        // EVERY item that beats the target is counted here; the user's history items among them are taken back below -- a scan of the (up to 264) history ids
        // per beating item was most of this loop (on random scores half the items beat the target: 36 TF/s = 0.23 of the fp32 MFMA rate, round 5)
        if constexpr (CAND) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) local[rr] += (i < N1 && c != 0 && acc[rr] > ts[rr]) ? 1 : 0;
        } else {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) local[rr] += (i < N1 && acc[rr] > ts[rr]) ? 1 : 0;
        }
    }
    // The history items: score(u, h) for the j-th history id of each of the 16 users by the SAME instruction sequence (B rows = those ids, the diagonal kept, as for
    // the target: an element's bits do not depend on the column it sits in), once per id -- a repeated id, the pad item 0 or an id outside the table counts nothing,
    // as a mask would.  Only the workgroup that owns the first item range does this (the others share its users).
    if (blockIdx.y == 0) {
        int mx = 0;
#pragma unroll
        for (int u = 0; u < 16; ++u) mx = max(mx, nhist[u]);
        for (int j = wave; j < mx; j += 4) {
            const int h = j < nhist[r16] ? hist[r16][j] : 0;
            bool ok = h >= 1 && h < N1 && u0 + r16 < U;
            for (int k = 0; k < j && ok; ++k) ok = hist[r16][k] != h;          // first occurrence only
            if constexpr (CAND) ok = ok && cand[h] != 0;                      // (a history id that is no candidate was never counted)
            const int hrow = ok ? h : 0;
            uint4 b[KS];
            frag_load<E>(b, item_emb, hrow, kg);
            const f32x4_t acc = score_tile<float>(ua, b);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                if (kg * 4 + rr == r16 && ok && acc[rr] > ts[rr]) atomicSub(&cnt[r16], 1);
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        int c = local[rr];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);     // over the 16 item columns
        if (r16 == 0 && c) atomicAdd(&cnt[kg * 4 + rr], c);
    }
    __syncthreads();
    if (tid < 16 && u0 + tid < U && cnt[tid]) atomicAdd(rank + u0 + tid, cnt[tid]);
}

__global__ void fill_i32_kernel(int32_t* p, int n, int v) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = v;
}

// the one launch path of both exports; cand is read by the CAND = true kernels only
template <bool CAND>
int eval_rank_launch(void* stream, const float* prec, const float* item_emb, const int32_t* target, const int32_t* hist_ptr,
                     const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E) {
    if (!prec || !item_emb || !target || !hist_ptr || !hist_idx || !rank || (CAND && !cand) || U <= 0 || N1 < 2) return A4R_EINVAL;
    if (!width_served(WidthsF32{}, E) || !aligned16(prec, item_emb)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(fill_i32_kernel, dim3((U + 255) / 256), dim3(256), 0, s, rank, U, 1);
    const dim3 grid((U + 15) / 16, sweep_ranges(U, N1));
    with_width(WidthsF32{}, E, [&](auto e) {
        hipLaunchKernelGGL((eval_rank_kernel<decltype(e)::value, CAND>), grid, dim3(256), 0, s, prec, item_emb, target, hist_ptr, hist_idx, rank, U, N1, cand);
    });
    return a4r_launch_status();
}

}  // namespace

extern "C" int a4r_eval_rank(void* stream, const float* prec, const float* item_emb, const int32_t* target,
                             const int32_t* hist_ptr, const int32_t* hist_idx, int32_t* rank, int U, int N1, int E) {
    return eval_rank_launch<false>(stream, prec, item_emb, target, hist_ptr, hist_idx, nullptr, rank, U, N1, E);
}

extern "C" int a4r_eval_rank_cand(void* stream, const float* prec, const float* item_emb, const int32_t* target,
                                  const int32_t* hist_ptr, const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E) {
    return eval_rank_launch<true>(stream, prec, item_emb, target, hist_ptr, hist_idx, cand, rank, U, N1, E);
}
