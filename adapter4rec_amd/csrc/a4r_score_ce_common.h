// What the two full-softmax cross-entropy heads share (a4r_score_ce.hip: fp32, 16 rows per workgroup; a4r_score_ce_bf16.hip: bf16, 64): the
// head's definitions, the running (max, sum of exp) and its merges, the range merge and the d_prec finish launches, the workspace layouts and
// the host's checks.  The scores themselves come from a4r_score_sweep.h.
//
//   trained(r) = log_mask[r] != 0 and 1 <= tgt[r] < N1;  count = #trained rows;  w[r] = trained ? 1 / count : 0
//   loss = sum_r w[r] (lse_r - s[r, tgt_r]);  count == 0: loss and every gradient are exactly 0
//   workspace, forward: one (max, sum, target score, -) quadruple per (range, row); backward: one fp32 [rows, E] partial of d_prec per range
#pragma once
#include "a4r_score_sweep.h"
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

// one more score s of a row into its running (m, l); the target's score is kept when this is its item
A4R_DEV void ce_online(float s, bool is_tgt, float& m, float& l, float& st) {
    const float d = s - m;                              // one exp per score: the smaller of (s, max) relative to the larger
    const float e = __expf(-fabsf(d));
    if (d > 0.f) { l = l * e + 1.f; m = s; } else l += e;
    if (is_tgt) st = s;
}

// The lanes' running triples -> one triple per (row, range) in the workspace: over the 16 item columns, then over the 4 waves in wave order.
// ROWS rows per workgroup; lane (r16, kg) holds the rows 16 rt + 4 kg + rr.
template <int ROWS>
A4R_DEV void ce_reduce_store(float (&m)[ROWS / 16][4], float (&l)[ROWS / 16][4], float (&st)[ROWS / 16][4], float (&red)[4][ROWS][3],
                             float* __restrict__ ws, int R, int r0) {
    const int tid = threadIdx.x, wave = tid >> 6, r16 = tid & 15, kg = (tid & 63) >> 4;
#pragma unroll
    for (int rt = 0; rt < ROWS / 16; ++rt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {           // (the target's score sits in one lane: the others add 0)
                const float m2 = __shfl_xor(m[rt][rr], o, 64), l2 = __shfl_xor(l[rt][rr], o, 64);
                lse_merge(m[rt][rr], l[rt][rr], m2, l2);
                st[rt][rr] += __shfl_xor(st[rt][rr], o, 64);
            }
            if (r16 == 0) {
                float* o = red[wave][rt * 16 + kg * 4 + rr];
                o[0] = m[rt][rr]; o[1] = l[rt][rr]; o[2] = st[rt][rr];
            }
        }
    __syncthreads();
    if (tid < ROWS && r0 + tid < R) {
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

// The d_prec partial of a workgroup's ROWS rows over its item range: the 4 waves' accumulators d[rt][n][rr] = D[row 16 rt + 4 kg + rr][column
// col(n, r16)] are added in LDS (dsh: [ROWS][E]) in wave order, then stored to the range's slab of the workspace.
template <int ROWS, int E, typename ColMap>
A4R_DEV void ce_rows_partial_store(const f32x4_t (&d)[ROWS / 16][E / 16], float* dsh, float* __restrict__ ws, int R, int r0, ColMap col) {
    const int tid = threadIdx.x, wave = tid >> 6, r16 = tid & 15, kg = (tid & 63) >> 4;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int rt = 0; rt < ROWS / 16; ++rt)
#pragma unroll
                for (int n = 0; n < E / 16; ++n)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        float* o = dsh + (rt * 16 + kg * 4 + rr) * E + col(n, r16);
                        *o = w == 0 ? d[rt][n][rr] : *o + d[rt][n][rr];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < ROWS * E; e += 256) {
        const int row = r0 + e / E;
        if (row < R) ws[((size_t)blockIdx.y * R + row) * E + (e % E)] = dsh[e];
    }
}

// d_prec[r] = g w[r] (the ranges' partials in range order - table[tgt_r]); exact zeros for the rows that are not trained
template <typename T>
__global__ void __launch_bounds__(256) ce_rows_finish_kernel(const float* __restrict__ ws, const T* __restrict__ table,
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
            v = gw * (s - Elem<T>::ld(table + (size_t)tg * E + e));
        }
        d_prec[idx] = v;
    }
}

// ---------------------------------------------------------------- host side
template <typename Ws> bool ce_shape_ok(Ws widths, int R, int N1, int E, int ranges) {
    return R > 0 && N1 >= 2 && width_served(widths, E) && ranges >= 0 && ranges <= MAX_RANGES;
}
// what every launch entry point refuses: a shape outside the head's, operands that are not 16-byte aligned
template <typename Ws> bool ce_args_ok(Ws widths, const void* prec, const void* table, int R, int N1, int E, int ranges) {
    return ce_shape_ok(widths, R, N1, E, ranges) && aligned16(prec, table);
}

// the library's range count: about two workgroups per CU over the row groups, at most MAX_RANGES and at most one range per 16-item tile
int ce_ranges(int R, int N1, int rows_per_workgroup) {
    const int gx = (R + rows_per_workgroup - 1) / rows_per_workgroup, ntiles = (N1 - 1 + 15) / 16;
    int gy = (2 * a4r_cu_count() + gx - 1) / gx;
    if (gy > MAX_RANGES) gy = MAX_RANGES;
    if (gy > ntiles) gy = ntiles;
    return gy < 1 ? 1 : gy;
}

// the backward's partials; the forward's quadruples fit in them
size_t ce_ws_bytes(int gy, int R, int E) { return (size_t)gy * (size_t)R * (size_t)E * sizeof(float); }

template <typename T>
void launch_ce_rows_finish(hipStream_t s, const float* ws, const T* table, const int32_t* tgt, const float* log_mask, const float* loss_ws,
                           float loss_scale, const float* loss_scale_dev, float* d_prec, int R, int N1, int E, int gy) {
    const size_t total = (size_t)R * E;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(ce_rows_finish_kernel<T>, dim3(blocks), dim3(256), 0, s, ws, table, tgt, log_mask, loss_ws, loss_scale, loss_scale_dev,
                       d_prec, R, N1, E, gy);
}

}  // namespace
