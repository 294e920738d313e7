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

// ---------------------------------------------------------------- scores from the bf16 MFMA (a4r_eval_rank_bf16, include/a4r_score_bf16.h)
// The kernel above at prec_b = bf16(prec), table_b = bf16(item_emb) (a4r_score_ce_bf16_cast's copies): score_tile<bf16_t>, E / 32 steps of
// v_mfma_f32_16x16x32_bf16 into a zeroed accumulator.  What changes beside the operand type:
//   Row sets.  A workgroup holds RS sets of 16 users as A fragments (RS x KS x 4 VGPRs; a bf16 row is half the registers of an fp32 one) and
//     runs RS score tiles on every table tile it loaded: the table is streamed once per 16 RS users, at half the bytes.  4 RS counters a lane.
//   Request ahead.  PD tiles in flight per wave, not one: RS bf16 score tiles are a few dozen MFMA cycles, far less than a cache request.
//     The PD slots are a ring written out by unrolling (slot j serves the tiles first + (j + PD n) tstep): no register moves.
//   Take-back.  As above, by the same instruction sequence, one row set after the other through the one 16-user history array in LDS (17 KB,
//     as in the fp32 kernel: it bounds nothing here, the registers allow fewer workgroups than it does), in the first item range only.
template <int E, int RS, int PD, bool CAND>
__global__ void __launch_bounds__(256) eval_rank_bf16_kernel(const bf16_t* __restrict__ prec, const bf16_t* __restrict__ table,
                                                             const int32_t* __restrict__ target, const int32_t* __restrict__ hist_ptr,
                                                             const int32_t* __restrict__ hist_idx, int32_t* __restrict__ rank, int U, int N1,
                                                             const uint8_t* __restrict__ cand) {
    constexpr int KS = E / 32;                       // chunk steps (bf16: 32 k per step)
    __shared__ int32_t hist[16][MAXH];
    __shared__ int32_t nhist[16];
    __shared__ float tscore[RS * 16];
    __shared__ int32_t cnt[RS * 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int u0 = blockIdx.x * (16 * RS);
    if (tid < RS * 16) cnt[tid] = 0;
    uint4 ua[RS][KS];                                // A operand: RS sets of 16 users
#pragma unroll
    for (int rs = 0; rs < RS; ++rs) {
        const int urow = min(u0 + rs * 16 + r16, U - 1);
        frag_load<E>(ua[rs], prec, urow, kg);
        uint4 b[KS];                                 // target scores: B rows = the set's target items, the diagonal kept
        frag_load<E>(b, table, target[urow], kg);
        const f32x4_t acc = score_tile<bf16_t>(ua[rs], b);
        if (wave == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
                if (kg * 4 + rr == r16) tscore[rs * 16 + r16] = acc[rr];
        }
    }
    __syncthreads();
    float ts[RS][4];
    int local[RS][4];
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) { ts[rs][rr] = tscore[rs * 16 + kg * 4 + rr]; local[rs][rr] = 0; }
    const int ntiles = (N1 - 1 + 15) / 16, tstep = gridDim.y * 4;
    const int first = blockIdx.y * 4 + wave;
    uint4 bn[PD][KS];
    [[maybe_unused]] uint8_t cn[PD];                 // CAND: the candidate byte of this lane's item in each requested tile
#pragma unroll
    for (int j = 0; j < PD; ++j) {
        const int irow = min(1 + min(first + j * tstep, ntiles - 1) * 16 + r16, N1 - 1);      // (past the end: the last tile again, never used)
        frag_load<E>(bn[j], table, irow, kg);
        if constexpr (CAND) cn[j] = cand[irow];
    }
    for (int tb = first; tb < ntiles; tb += PD * tstep) {
#pragma unroll
        for (int j = 0; j < PD; ++j) {
            const int t = tb + j * tstep;
            if (t < ntiles) {
                const int i = 1 + t * 16 + r16;          // this lane's item column
                uint4 b[KS];
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) b[ks] = bn[j][ks];
                [[maybe_unused]] uint8_t c = 0;
                if constexpr (CAND) c = cn[j];
                {
                    const int irow = min(1 + min(t + PD * tstep, ntiles - 1) * 16 + r16, N1 - 1);
                    frag_load<E>(bn[j], table, irow, kg);
                    if constexpr (CAND) cn[j] = cand[irow];
                }
                const bool col = CAND ? (i < N1 && c != 0) : i < N1;
#pragma unroll
                for (int rs = 0; rs < RS; ++rs) {
                    const f32x4_t acc = score_tile<bf16_t>(ua[rs], b);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) local[rs][rr] += (col && acc[rr] > ts[rs][rr]) ? 1 : 0;
                }
            }
        }
    }
    // the history items, as in eval_rank_kernel: every counted item above, the user's own (first occurrence, inside the table, a candidate) taken back
    if (blockIdx.y == 0) {
#pragma unroll
        for (int rs = 0; rs < RS; ++rs) {
            __syncthreads();                         // (the set before this one has been read)
            {
                const int ul = tid >> 4, u = min(u0 + rs * 16 + ul, U - 1);
                const int b = hist_ptr[u], n = max(0, min(hist_ptr[u + 1] - b, MAXH));
                for (int j = tid & 15; j < n; j += 16) hist[ul][j] = hist_idx[b + j];
                if ((tid & 15) == 0) nhist[ul] = n;
            }
            __syncthreads();
            int mx = 0;
#pragma unroll
            for (int u = 0; u < 16; ++u) mx = max(mx, nhist[u]);
            for (int j = wave; j < mx; j += 4) {
                const int h = j < nhist[r16] ? hist[r16][j] : 0;
                bool ok = h >= 1 && h < N1 && u0 + rs * 16 + r16 < U;
                for (int k = 0; k < j && ok; ++k) ok = hist[r16][k] != h;          // first occurrence only
                if constexpr (CAND) ok = ok && cand[ok ? h : 0] != 0;
                const int hrow = ok ? h : 0;
                uint4 b[KS];
                frag_load<E>(b, table, hrow, kg);
                const f32x4_t acc = score_tile<bf16_t>(ua[rs], b);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    if (kg * 4 + rr == r16 && ok && acc[rr] > ts[rs][rr]) atomicSub(&cnt[rs * 16 + r16], 1);
            }
        }
    }
#pragma unroll
    for (int rs = 0; rs < RS; ++rs)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int c = local[rs][rr];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);     // over the 16 item columns
            if (r16 == 0 && c) atomicAdd(&cnt[rs * 16 + kg * 4 + rr], c);
        }
    __syncthreads();
    if (tid < RS * 16 && u0 + tid < U && cnt[tid]) atomicAdd(rank + u0 + tid, cnt[tid]);
}

// Row sets and tiles in flight per width, from the compiler's report and from timings (DESIGN section 7 has both): 128 / 128 / 64 / 32 users a
// workgroup, the A fragments 64 / 128 / 128 / 128 VGPRs.  The sweep is bound by the table's bytes from the cache at every width, so each
// doubling of RS that still compiles without scratch was faster (E = 128 runs one wave per SIMD at 256 VGPRs and is faster than RS = 4 at
// three); a third tile in flight bought nothing measurable once two were, and at E = 256 / 512 the registers go to row sets instead.
template <int E> struct RankBf16Shape {
    static constexpr int RS = E <= 128 ? 8 : E == 256 ? 4 : 2;
    static constexpr int PD = E <= 128 ? 2 : 1;
};

template <bool CAND>
void eval_rank_bf16_launch(hipStream_t s, const bf16_t* prec, const bf16_t* table, const int32_t* target, const int32_t* hist_ptr,
                           const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E) {
    hipLaunchKernelGGL(fill_i32_kernel, dim3((U + 255) / 256), dim3(256), 0, s, rank, U, 1);
    with_width(WidthsF32{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value, RS = RankBf16Shape<W>::RS, PD = RankBf16Shape<W>::PD;
        const int sets = (U + RS - 1) / RS;          // sweep_ranges over workgroups of 16 RS users
        const dim3 grid((sets + 15) / 16, sweep_ranges(sets, N1));
        hipLaunchKernelGGL((eval_rank_bf16_kernel<W, RS, PD, CAND>), grid, dim3(256), 0, s, prec, table, target, hist_ptr, hist_idx, rank, U, N1, cand);
    });
}

}  // namespace

extern "C" int a4r_eval_rank_bf16(void* stream, const void* prec_b, const void* table_b, const int32_t* target, const int32_t* hist_ptr,
                                  const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E) {
    if (!prec_b || !table_b || !target || !hist_ptr || !hist_idx || !rank || U <= 0 || N1 < 2) return A4R_EINVAL;
    if (!width_served(WidthsF32{}, E) || !aligned16(prec_b, table_b)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    if (cand) eval_rank_bf16_launch<true>(s, prec, table, target, hist_ptr, hist_idx, cand, rank, U, N1, E);
    else eval_rank_bf16_launch<false>(s, prec, table, target, hist_ptr, hist_idx, nullptr, rank, U, N1, E);
    return a4r_launch_status();
}

extern "C" int a4r_eval_rank(void* stream, const float* prec, const float* item_emb, const int32_t* target,
                             const int32_t* hist_ptr, const int32_t* hist_idx, int32_t* rank, int U, int N1, int E) {
    return eval_rank_launch<false>(stream, prec, item_emb, target, hist_ptr, hist_idx, nullptr, rank, U, N1, E);
}

extern "C" int a4r_eval_rank_cand(void* stream, const float* prec, const float* item_emb, const int32_t* target,
                                  const int32_t* hist_ptr, const int32_t* hist_idx, const uint8_t* cand, int32_t* rank, int U, int N1, int E) {
    return eval_rank_launch<true>(stream, prec, item_emb, target, hist_ptr, hist_idx, cand, rank, U, N1, E);
}
