// Full-softmax cross-entropy head of the ID tower (--loss ce): every trained row r = (user, position) against the whole item table, without
// ever forming the [rows, items] logits.
//
//   s[r, i] = <prec[r], table[i]>, i = 1 .. N (row 0 of the table is the pad row: never a candidate), lse_r = log sum_i exp s[r, i]
//   trained(r), count, w[r] and the loss: a4r_score_ce_common.h
//
// Scores come from the item-table score sweep (a4r_score_sweep.h), fp32, 16 rows per workgroup, requested one tile ahead where the registers
// allow it (PF below).
//
// Forward.  Every lane keeps a running (max, sum of exp) for its 4 rows over its item column and picks up s[r, tgt_r] when the target is its
// item; the 16 columns, then the 4 waves (in order), are merged and one (max, sum, target score) triple per (row, range) goes to the workspace.
// A one-workgroup merge launch folds the ranges in range order into lse and s_tgt, counts the trained rows and sums the loss (fp64, fixed order).
//
// Backward recomputes the scores from prec, table and the saved lse (p = exp(s - lse)), twice:
//   rows:   d_prec[r] = g w[r] (sum_i p[r, i] table[i] - table[tgt_r]).  The score tile is formed TRANSPOSED (item tile as A, rows as B), so that
//           the accumulator a lane holds -- p[row = lane & 15][item = 4 (lane >> 4) + reg] -- is the A fragment of the second product as it
//           stands; its B fragments (table[item][16 n + column]) are read again from the tile just streamed (L1 / L2).  Per-range partials go
//           to the workspace, a second launch adds them in range order, subtracts the target row and scales.
//   items:  d_table[i] += g sum_r w[r] (p[r, i] - [i == tgt_r]) prec[r].  A wave owns an item tile (its B fragments stay in registers) and walks
//           all rows in ascending tiles of 16; the score accumulator -- (row = 4 (lane >> 4) + reg, item = lane & 15) -- is the A fragment
//           of the second product (contraction over rows).  Every table row is written by exactly one wave, once.
// No float atomics and a fixed schedule: the same inputs give the same bits on every call.  Nothing of size rows x items is written anywhere.
#include "a4r_score_ce_common.h"

namespace {

// PF = false at E = 512: rows, tile and next tile would be 3 x 128 registers a lane and one workgroup per CU; without the request the kernel
// fits 256 registers and two workgroups share a CU.
template <int E, bool PF>
__global__ void __launch_bounds__(256) ce_fwd_kernel(const float* __restrict__ prec, const float* __restrict__ table,
                                                     const int32_t* __restrict__ tgt, float* __restrict__ ws, int R, int N1) {
    constexpr int KS = E / 16;
    __shared__ float red[4][16][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int r0 = blockIdx.x * 16;
    uint4 ua[KS];
    frag_load<E>(ua, prec, min(r0 + r16, R - 1), kg);
    int tg[4];
    float m[1][4], l[1][4], st[1][4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = r0 + kg * 4 + rr;
        tg[rr] = row < R ? tgt[row] : 0;
        m[0][rr] = -__builtin_huge_valf(); l[0][rr] = 0.f; st[0][rr] = 0.f;
    }
    const SweepDeal<> deal(N1, wave);
    uint4 bn[PF ? KS : 1];
    sweep_begin<E, PF>(bn, table, deal, r16, kg);
    for (int t = deal.first; t < deal.ntiles; t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column
        uint4 b[KS];
        sweep_next<E, PF>(b, bn, table, deal, t, r16, kg);
        const f32x4_t acc = score_tile<float>(ua, b);
        if (i < N1) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) ce_online(acc[rr], i == tg[rr], m[0][rr], l[0][rr], st[0][rr]);
        }
    }
    ce_reduce_store<16>(m, l, st, red, ws, R, r0);
}

// PF up to E = 128; wider rows keep the registers for the E / 4 output accumulators
template <int E, bool PF>
__global__ void __launch_bounds__(256) ce_bwd_rows_kernel(const float* __restrict__ prec, const float* __restrict__ table,
                                                          const float* __restrict__ lse, float* __restrict__ ws, int R, int N1) {
    constexpr int KS = E / 16, NT = E / 16;
    extern __shared__ float dsh[];                   // [16][E]: the 4 waves' partial sums, added in wave order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int r0 = blockIdx.x * 16;
    uint4 ua[KS];
    const int urow = min(r0 + r16, R - 1);
    frag_load<E>(ua, prec, urow, kg);
    const float lse_r = lse[urow];
    f32x4_t d[1][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) d[0][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const SweepDeal<> deal(N1, wave);
    uint4 bn[PF ? KS : 1];
    sweep_begin<E, PF>(bn, table, deal, r16, kg);
    for (int t = deal.first; t < deal.ntiles; t += deal.tstep) {
        uint4 b[KS];
        sweep_next<E, PF>(b, bn, table, deal, t, r16, kg);
        const f32x4_t acc = score_tile<float>(b, ua);   // transposed tile: acc[rr] = s[row r16][item 4 kg + rr]
        const int i0 = 1 + t * 16 + kg * 4;
        float p[4];
        const float* brow[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            p[rr] = i0 + rr < N1 ? __expf(acc[rr] - lse_r) : 0.f;
            brow[rr] = table + (size_t)min(i0 + rr, N1 - 1) * E + r16;
        }
        const uint4 pa = Elem<float>::pack(p);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            float bv[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) bv[rr] = brow[rr][n * 16];
            Mma<float>::mma(pa, Elem<float>::pack(bv), d[0][n]);      // d[0][n][rr] = D[row 4 kg + rr][column 16 n + r16]
        }
    }
    ce_rows_partial_store<16, E>(d, dsh, ws, R, r0, [](int n, int c) { return n * 16 + c; });
}

// PF: the next ROW tile's fragments are requested one tile ahead (E <= 128, as ce_bwd_rows_kernel)
template <int E, bool PF>
__global__ void __launch_bounds__(256) ce_bwd_items_kernel(const float* __restrict__ prec, const float* __restrict__ table,
                                                           const int32_t* __restrict__ tgt, const float* __restrict__ log_mask,
                                                           const float* __restrict__ lse, const float* __restrict__ loss_ws, float loss_scale,
                                                           const float* __restrict__ loss_scale_dev, float* __restrict__ d_table, int ldg, int R,
                                                           int N1) {
    constexpr int KS = E / 16, NT = E / 16;
    const float gw = ce_gw(loss_ws, loss_scale, loss_scale_dev);
    if (gw == 0.f) return;                               // no trained row (or a zero incoming gradient): the destination keeps its bits
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int ntiles = (N1 - 1 + 15) / 16, rtiles = (R + 15) / 16;
    for (int t = blockIdx.x * 4 + wave; t < ntiles; t += gridDim.x * 4) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column of the score tile
        uint4 b[KS];
        frag_load<E>(b, table, min(i, N1 - 1), kg);
        f32x4_t d[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) d[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        uint4 an[PF ? KS : 1];
        if constexpr (PF) frag_load<E>(an, prec, min(r16, R - 1), kg);
        for (int rt = 0; rt < rtiles; ++rt) {
            const int r0 = rt * 16;
            uint4 ua[KS];
            if constexpr (PF) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ua[ks] = an[ks];
                frag_load<E>(an, prec, min(min(rt + 1, rtiles - 1) * 16 + r16, R - 1), kg);
            } else {
                frag_load<E>(ua, prec, min(r0 + r16, R - 1), kg);
            }
            const f32x4_t acc = score_tile<float>(ua, b);       // acc[rr] = s[row r0 + 4 kg + rr][item i]
            float c[4];
            const float* arow[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = r0 + kg * 4 + rr, rc = min(row, R - 1);
                const int tg = tgt[rc];
                const bool on = row < R && ce_trained(log_mask, tg, rc, N1);
                c[rr] = on ? __expf(acc[rr] - lse[rc]) - (i == tg ? 1.f : 0.f) : 0.f;
                arow[rr] = prec + (size_t)rc * E + r16;
            }
            const uint4 ca = Elem<float>::pack(c);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                float bv[4];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) bv[rr] = arow[rr][n * 16];
                Mma<float>::mma(ca, Elem<float>::pack(bv), d[n]);      // d[n][rr] = G[item 4 kg + rr of the tile][column 16 n + r16]
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int item = 1 + t * 16 + kg * 4 + rr;
            if (item < N1) {
                float* o = d_table + (size_t)item * ldg + r16;
#pragma unroll
                for (int n = 0; n < NT; ++n) o[n * 16] += gw * d[n][rr];
            }
        }
    }
}

}  // namespace

extern "C" int a4r_score_ce_ranges(int R, int N1) {
    if (R <= 0 || N1 < 2) return A4R_EINVAL;
    return ce_ranges(R, N1, 16);
}

extern "C" size_t a4r_score_ce_ws_bytes(int R, int N1, int E, int ranges) {
    if (!ce_shape_ok(WidthsF32{}, R, N1, E, ranges)) return 0;
    return ce_ws_bytes(ranges ? ranges : ce_ranges(R, N1, 16), R, E);
}

extern "C" int a4r_score_ce_fwd(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask, float* lse,
                                float* s_tgt, float* loss_ws, void* ws, int R, int N1, int E, int ranges) {
    if (!prec || !table || !tgt || !log_mask || !lse || !s_tgt || !loss_ws || !ws || !ce_args_ok(WidthsF32{}, prec, table, R, N1, E, ranges)) return A4R_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 15u) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int gy = ranges ? ranges : ce_ranges(R, N1, 16);
    const dim3 grid((R + 15) / 16, gy);
    float* w = static_cast<float*>(ws);
    with_width(WidthsF32{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        hipLaunchKernelGGL((ce_fwd_kernel<W, W <= 256>), grid, dim3(256), 0, s, prec, table, tgt, w, R, N1);
    });
    hipLaunchKernelGGL(ce_merge_kernel, dim3(1), dim3(256), 0, s, w, tgt, log_mask, lse, s_tgt, loss_ws, R, N1, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bwd_rows(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask,
                                     const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_prec,
                                     void* ws, int R, int N1, int E, int ranges) {
    if (!prec || !table || !tgt || !log_mask || !lse || !loss_ws || !d_prec || !ws || !ce_args_ok(WidthsF32{}, prec, table, R, N1, E, ranges)) return A4R_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 15u) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int gy = ranges ? ranges : ce_ranges(R, N1, 16);
    const dim3 grid((R + 15) / 16, gy);
    float* w = static_cast<float*>(ws);
    int rc = A4R_OK;
    with_width(WidthsF32{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        const auto kernel = ce_bwd_rows_kernel<W, W <= 128>;
        const size_t lds = (size_t)16 * W * sizeof(float);
        if ((rc = a4r_set_lds(kernel, lds))) return;
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, prec, table, lse, w, R, N1);
    });
    if (rc) return rc;
    launch_ce_rows_finish(s, w, table, tgt, log_mask, loss_ws, loss_scale, loss_scale_dev, d_prec, R, N1, E, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bwd_items(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask,
                                      const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table,
                                      int ldg, int R, int N1, int E) {
    if (!prec || !table || !tgt || !log_mask || !lse || !loss_ws || !d_table || !ce_args_ok(WidthsF32{}, prec, table, R, N1, E, 0) || ldg < E) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ntiles = (N1 - 1 + 15) / 16;
    int grid = (ntiles + 3) / 4;
    const int cap = 8 * a4r_cu_count();
    if (grid > cap) grid = cap;
    with_width(WidthsF32{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        hipLaunchKernelGGL((ce_bwd_items_kernel<W, W <= 128>), dim3(grid), dim3(256), 0, s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale,
                           loss_scale_dev, d_table, ldg, R, N1);
    });
    return a4r_launch_status();
}
