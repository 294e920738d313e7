// Full-softmax cross-entropy head of the ID tower (--loss ce): every trained row r = (user, position) against the whole item table, without
// ever forming the [rows, items] logits.
//
//   s[r, i] = <prec[r], table[i]>, i = 1 .. N (row 0 of the table is the pad row: never a candidate), lse_r = log sum_i exp s[r, i]
//   trained(r) = log_mask[r] != 0 and 1 <= tgt[r] < N1;  count = #trained rows;  w[r] = trained ? 1 / count : 0
//   loss = sum_r w[r] (lse_r - s[r, tgt_r]);  count == 0: loss and every gradient are exactly 0
//
// Scores are formed as a4r_topk_items forms them (a4r_topk.hip): 16 rows per workgroup as the A operand of fp32 MFMA 16x16x4 tiles held in
// registers, the table streamed 16 rows at a time as the B operand with the next tile's fragments requested one tile ahead (E <= 256), the 4 waves of a
// workgroup taking every 4th tile of the workgroup's item range (range y of gy owns tiles 4 y + wave + 4 gy k).
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
#include "a4r_common.h"
#include "../../include/a4r.h"

namespace {

constexpr int MAX_RANGES = A4R_SCORE_CE_MAX_RANGES;

// (m, l) <- the (max, sum of exp(s - max)) pair of the union of two score sets; an empty set is (-inf, 0) and merges without a NaN
A4R_DEV void lse_merge(float& m, float& l, float m2, float l2) {
    const float mn = fmaxf(m, m2);
    const float a = m == mn ? l : l * __expf(m - mn);
    const float b = m2 == mn ? l2 : l2 * __expf(m2 - mn);
    m = mn;
    l = a + b;
}

A4R_DEV bool ce_trained(const float* __restrict__ log_mask, int tg, int r, int N1) { return log_mask[r] != 0.f && tg >= 1 && tg < N1; }

// g / count, 0 when no row is trained
A4R_DEV float ce_gw(const float* __restrict__ loss_ws, float loss_scale, const float* __restrict__ loss_scale_dev) {
    const float cnt = loss_ws[2];
    return cnt > 0.f ? loss_scale * (loss_scale_dev ? loss_scale_dev[0] : 1.f) / cnt : 0.f;
}

// PF: the next tile's fragments are requested one tile ahead, as topk_partial_kernel does.  E = 512 goes without: rows, tile and next tile would be
// 3 x 128 registers a lane and one workgroup per CU; without the request the kernel fits 256 registers and two workgroups share a CU.
template <int E, bool PF>
__global__ void __launch_bounds__(256) ce_fwd_kernel(const float* __restrict__ prec, const float* __restrict__ table,
                                                     const int32_t* __restrict__ tgt, float* __restrict__ ws, int R, int N1) {
    constexpr int KS = E / 16;
    __shared__ float red[4][16][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int r0 = blockIdx.x * 16;
    uint4 ua[KS];
    const int urow = min(r0 + r16, R - 1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) ua[ks] = *reinterpret_cast<const uint4*>(prec + (size_t)urow * E + (ks * 4 + kg) * 4);
    int tg[4];
    float m[4], l[4], st[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = r0 + kg * 4 + rr;
        tg[rr] = row < R ? tgt[row] : 0;
        m[rr] = -__builtin_huge_valf(); l[rr] = 0.f; st[rr] = 0.f;
    }
    const int ntiles = (N1 - 1 + 15) / 16, tstep = gridDim.y * 4;
    int t = blockIdx.y * 4 + wave;
    uint4 bn[PF ? KS : 1];
    if constexpr (PF) {
        const int irow = min(1 + min(t, ntiles - 1) * 16 + r16, N1 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
    }
    for (; t < ntiles; t += tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column
        uint4 b[KS];
        if constexpr (PF) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = bn[ks];
            const int irow = min(1 + min(t + tstep, ntiles - 1) * 16 + r16, N1 - 1);      // (past the end: the last tile again, never used)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
        } else {
            const int irow = min(i, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Mma<float>::mma(ua[ks], b[ks], acc);
        if (i < N1) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float s = acc[rr], d = s - m[rr];         // one exp per score: the smaller of (s, max) relative to the larger
                const float e = __expf(-fabsf(d));
                if (d > 0.f) { l[rr] = l[rr] * e + 1.f; m[rr] = s; } else l[rr] += e;
                if (i == tg[rr]) st[rr] = s;
            }
        }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {               // over the 16 item columns (the target's score sits in one lane: the others add 0)
            const float m2 = __shfl_xor(m[rr], o, 64), l2 = __shfl_xor(l[rr], o, 64);
            lse_merge(m[rr], l[rr], m2, l2);
            st[rr] += __shfl_xor(st[rr], o, 64);
        }
        if (r16 == 0) { red[wave][kg * 4 + rr][0] = m[rr]; red[wave][kg * 4 + rr][1] = l[rr]; red[wave][kg * 4 + rr][2] = st[rr]; }
    }
    __syncthreads();
    if (tid < 16 && r0 + tid < R) {
        float mm = red[0][tid][0], ll = red[0][tid][1], ss = red[0][tid][2];
#pragma unroll
        for (int w = 1; w < 4; ++w) { lse_merge(mm, ll, red[w][tid][0], red[w][tid][1]); ss += red[w][tid][2]; }
        float* o = ws + ((size_t)blockIdx.y * R + r0 + tid) * 4;
        o[0] = mm; o[1] = ll; o[2] = ss;
    }
}

// one workgroup: the ranges of every row in range order -> lse, s_tgt; the trained rows counted, their losses summed in fp64 in a fixed order
__global__ void __launch_bounds__(256) ce_merge_kernel(const float* __restrict__ ws, const int32_t* __restrict__ tgt,
                                                       const float* __restrict__ log_mask, float* __restrict__ lse, float* __restrict__ s_tgt,
                                                       float* __restrict__ loss_ws, int R, int N1, int gy) {
    __shared__ double wsum[4];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x;
    double sum = 0.0;
    int cnt = 0;
    for (int r = tid; r < R; r += 256) {
        float m = -__builtin_huge_valf(), l = 0.f, st = 0.f;
        for (int y = 0; y < gy; ++y) {
            const float* p = ws + ((size_t)y * R + r) * 4;
            lse_merge(m, l, p[0], p[1]);
            st += p[2];
        }
        const float v = m + logf(l);
        lse[r] = v;
        s_tgt[r] = st;
        if (ce_trained(log_mask, tgt[r], r, N1)) { sum += (double)v - (double)st; ++cnt; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if ((tid & 63) == 0) { wsum[tid >> 6] = sum; wcnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        const double tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        const int n = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        loss_ws[0] = n ? (float)(tot / n) : 0.f;
        loss_ws[1] = n ? (float)tot : 0.f;
        loss_ws[2] = (float)n;
    }
}

// PF: the next tile's fragments are requested one tile ahead (E <= 128; wider rows keep the registers for the E / 4 output accumulators)
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
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) ua[ks] = *reinterpret_cast<const uint4*>(prec + (size_t)urow * E + (ks * 4 + kg) * 4);
    const float lse_r = lse[urow];
    f32x4_t d[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) d[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (N1 - 1 + 15) / 16, tstep = gridDim.y * 4;
    int t = blockIdx.y * 4 + wave;
    uint4 bn[PF ? KS : 1];
    if constexpr (PF) {
        const int irow = min(1 + min(t, ntiles - 1) * 16 + r16, N1 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
    }
    for (; t < ntiles; t += tstep) {
        uint4 b[KS];
        if constexpr (PF) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = bn[ks];
            const int irow = min(1 + min(t + tstep, ntiles - 1) * 16 + r16, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bn[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
        } else {
            const int irow = min(1 + t * 16 + r16, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
        }
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};             // transposed tile: acc[rr] = s[row r16][item 4 kg + rr]
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) Mma<float>::mma(b[ks], ua[ks], acc);
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
            Mma<float>::mma(pa, Elem<float>::pack(bv), d[n]);      // d[n][rr] = D[row 4 kg + rr][column 16 n + r16]
        }
    }
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    float* o = dsh + (kg * 4 + rr) * E + n * 16 + r16;
                    *o = w == 0 ? d[n][rr] : *o + d[n][rr];
                }
        }
        __syncthreads();
    }
    for (int e = tid; e < 16 * E; e += 256) {
        const int row = r0 + e / E;
        if (row < R) ws[((size_t)blockIdx.y * R + row) * E + (e % E)] = dsh[e];
    }
}

// d_prec[r] = g w[r] (the ranges' partials in range order - table[tgt_r]); exact zeros for the rows that are not trained
__global__ void __launch_bounds__(256) ce_rows_finish_kernel(const float* __restrict__ ws, const float* __restrict__ table,
                                                             const int32_t* __restrict__ tgt, const float* __restrict__ log_mask,
                                                             const float* __restrict__ loss_ws, float loss_scale,
                                                             const float* __restrict__ loss_scale_dev, float* __restrict__ d_prec, int R, int N1,
                                                             int E, int gy) {
    const float gw = ce_gw(loss_ws, loss_scale, loss_scale_dev);
    const size_t total = (size_t)R * E;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int r = (int)(idx / E), e = (int)(idx % E);
        const int tg = tgt[r];
        float v = 0.f;
        if (gw != 0.f && ce_trained(log_mask, tg, r, N1)) {
            float s = 0.f;
            for (int y = 0; y < gy; ++y) s += ws[(size_t)y * total + idx];
            v = gw * (s - table[(size_t)tg * E + e]);
        }
        d_prec[idx] = v;
    }
}

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
        {
            const int irow = min(i, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[ks] = *reinterpret_cast<const uint4*>(table + (size_t)irow * E + (ks * 4 + kg) * 4);
        }
        f32x4_t d[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) d[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        uint4 an[PF ? KS : 1];
        if constexpr (PF) {
            const int urow = min(r16, R - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[ks] = *reinterpret_cast<const uint4*>(prec + (size_t)urow * E + (ks * 4 + kg) * 4);
        }
        for (int rt = 0; rt < rtiles; ++rt) {
            const int r0 = rt * 16;
            uint4 ua[KS];
            if constexpr (PF) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ua[ks] = an[ks];
                const int urow = min(min(rt + 1, rtiles - 1) * 16 + r16, R - 1);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) an[ks] = *reinterpret_cast<const uint4*>(prec + (size_t)urow * E + (ks * 4 + kg) * 4);
            } else {
                const int urow = min(r0 + r16, R - 1);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ua[ks] = *reinterpret_cast<const uint4*>(prec + (size_t)urow * E + (ks * 4 + kg) * 4);
            }
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};         // acc[rr] = s[row r0 + 4 kg + rr][item i]
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Mma<float>::mma(ua[ks], b[ks], acc);
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

bool ce_width_ok(int E) { return E == 64 || E == 128 || E == 256 || E == 512; }
bool ce_shape_ok(int R, int N1, int E, int ranges) { return R > 0 && N1 >= 2 && ce_width_ok(E) && ranges >= 0 && ranges <= MAX_RANGES; }

// the library's range count: about two workgroups per CU over the row tiles, at most MAX_RANGES and at most one range per 16-item tile
int ce_ranges(int R, int N1) {
    const int gx = (R + 15) / 16, ntiles = (N1 - 1 + 15) / 16;
    int gy = (2 * a4r_cu_count() + gx - 1) / gx;
    if (gy > MAX_RANGES) gy = MAX_RANGES;
    if (gy > ntiles) gy = ntiles;
    return gy < 1 ? 1 : gy;
}

template <int E> void launch_fwd(hipStream_t s, dim3 grid, const float* prec, const float* table, const int32_t* tgt, float* ws, int R, int N1) {
    hipLaunchKernelGGL((ce_fwd_kernel<E, E <= 256>), grid, dim3(256), 0, s, prec, table, tgt, ws, R, N1);
}
template <int E> int launch_rows(hipStream_t s, dim3 grid, const float* prec, const float* table, const float* lse, float* ws, int R, int N1) {
    constexpr bool PF = E <= 128;
    const size_t lds = (size_t)16 * E * sizeof(float);
    if (int rc = a4r_set_lds(ce_bwd_rows_kernel<E, PF>, lds)) return rc;
    hipLaunchKernelGGL((ce_bwd_rows_kernel<E, PF>), grid, dim3(256), lds, s, prec, table, lse, ws, R, N1);
    return A4R_OK;
}
template <int E> void launch_items(hipStream_t s, int grid, const float* prec, const float* table, const int32_t* tgt, const float* log_mask,
                                   const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table, int ldg,
                                   int R, int N1) {
    constexpr bool PF = E <= 128;
    hipLaunchKernelGGL((ce_bwd_items_kernel<E, PF>), dim3(grid), dim3(256), 0, s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale,
                       loss_scale_dev, d_table, ldg, R, N1);
}

bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

}  // namespace

extern "C" int a4r_score_ce_ranges(int R, int N1) {
    if (R <= 0 || N1 < 2) return A4R_EINVAL;
    return ce_ranges(R, N1);
}

extern "C" size_t a4r_score_ce_ws_bytes(int R, int N1, int E, int ranges) {
    if (!ce_shape_ok(R, N1, E, ranges)) return 0;
    const int gy = ranges ? ranges : ce_ranges(R, N1);
    return (size_t)gy * (size_t)R * (size_t)E * sizeof(float);          // the backward's partials; the forward's triples (4 floats a row) fit in it
}

extern "C" int a4r_score_ce_fwd(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask, float* lse,
                                float* s_tgt, float* loss_ws, void* ws, int R, int N1, int E, int ranges) {
    if (!prec || !table || !tgt || !log_mask || !lse || !s_tgt || !loss_ws || !ws || !ce_shape_ok(R, N1, E, ranges)) return A4R_EINVAL;
    if (!aligned16(prec, table) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int gy = ranges ? ranges : ce_ranges(R, N1);
    const dim3 grid((R + 15) / 16, gy);
    float* w = static_cast<float*>(ws);
    if (E == 64) launch_fwd<64>(s, grid, prec, table, tgt, w, R, N1);
    else if (E == 128) launch_fwd<128>(s, grid, prec, table, tgt, w, R, N1);
    else if (E == 256) launch_fwd<256>(s, grid, prec, table, tgt, w, R, N1);
    else launch_fwd<512>(s, grid, prec, table, tgt, w, R, N1);
    hipLaunchKernelGGL(ce_merge_kernel, dim3(1), dim3(256), 0, s, w, tgt, log_mask, lse, s_tgt, loss_ws, R, N1, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bwd_rows(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask,
                                     const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_prec,
                                     void* ws, int R, int N1, int E, int ranges) {
    if (!prec || !table || !tgt || !log_mask || !lse || !loss_ws || !d_prec || !ws || !ce_shape_ok(R, N1, E, ranges)) return A4R_EINVAL;
    if (!aligned16(prec, table) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int gy = ranges ? ranges : ce_ranges(R, N1);
    const dim3 grid((R + 15) / 16, gy);
    float* w = static_cast<float*>(ws);
    int rc;
    if (E == 64) rc = launch_rows<64>(s, grid, prec, table, lse, w, R, N1);
    else if (E == 128) rc = launch_rows<128>(s, grid, prec, table, lse, w, R, N1);
    else if (E == 256) rc = launch_rows<256>(s, grid, prec, table, lse, w, R, N1);
    else rc = launch_rows<512>(s, grid, prec, table, lse, w, R, N1);
    if (rc) return rc;
    const size_t total = (size_t)R * E;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(ce_rows_finish_kernel, dim3(blocks), dim3(256), 0, s, w, table, tgt, log_mask, loss_ws, loss_scale, loss_scale_dev, d_prec,
                       R, N1, E, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bwd_items(void* stream, const float* prec, const float* table, const int32_t* tgt, const float* log_mask,
                                      const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table,
                                      int ldg, int R, int N1, int E) {
    if (!prec || !table || !tgt || !log_mask || !lse || !loss_ws || !d_table || !ce_shape_ok(R, N1, E, 0) || ldg < E) return A4R_EINVAL;
    if (!aligned16(prec, table)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int ntiles = (N1 - 1 + 15) / 16;
    int grid = (ntiles + 3) / 4;
    const int cap = 8 * a4r_cu_count();
    if (grid > cap) grid = cap;
    if (E == 64) launch_items<64>(s, grid, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    else if (E == 128) launch_items<128>(s, grid, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    else if (E == 256) launch_items<256>(s, grid, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    else launch_items<512>(s, grid, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    return a4r_launch_status();
}
