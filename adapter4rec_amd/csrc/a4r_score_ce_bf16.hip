// The full-softmax cross-entropy head of the ID tower on the bf16 MFMA (--ce_dtype bf16): the function of a4r_score_ce.hip evaluated at
// prec_b = bf16(prec), table_b = bf16(table) (round to nearest even; a4r_score_ce_bf16_cast writes the two copies), scores accumulated in fp32.
//
//   s[r, i] = <prec_b[r], table_b[i]>, i = 1 .. N1-1;  lse, s_tgt, loss, count, trained(r), w[r] as a4r_score_ce.hip states them
//   d_prec[r]  = g w[r] (sum_i p[r, i] table_b[i] - table_b[tgt_r])                 (straight-through: handed to the fp32 masters as it is)
//   d_table[i] += g sum_r w[r] (p[r, i] - [i == tgt_r]) prec_b[r]
//
// Why not the fp32 kernels with another Mma: at a large table they are bound by the bytes of a table pass as much as by the MFMA (every 16-row
// workgroup streams its whole item range).  Here a workgroup holds G = 64 rows -- each wave keeps the G / 16 = 4 row tiles of prec_b as A
// fragments (8 VGPRs a tile at E = 64) -- and a 16-item tile's B fragments, loaded once, meet all four: a quarter of the table passes at half
// the bytes a pass.  One v_mfma_f32_16x16x32_bf16 covers K = 32 (a lane's 16-byte chunk is 8 elements, k = 8 (lane >> 4) + j).
//
// Forward: as ce_fwd_kernel, four row tiles wide.  Range merge: the same one-workgroup launch.
// Backward, rows:  the score tiles of TWO 16-item tiles are formed transposed (items as A, rows as B): a lane then holds p[row = lane & 15] for
//   the items 4 kg + reg of either tile, which is the K = 32 A fragment of the second product under the contraction order
//       slot 8 kg + j  <->  item 32 u + 16 (j >> 2) + 4 kg + (j & 3) of pair u        (a permutation of the pair's 32 items)
//   p is rounded to bf16 there (the one approximation besides the operands).  The B fragments follow the same order: a lane reads, for each
//   of its 8 items, the DWORD that holds columns 32 q + 2 (lane & 15) and + 1; the low halves are the fragment of one 16-column tile and the
//   high halves that of the next, so output tile n' = 2 q + h holds the columns 32 q + 2 (lane & 15) + h.  8 loads feed 2 x 4 MFMAs.
// Backward, items: a wave owns IT item tiles (B fragments in registers) and walks all rows 32 at a time; the score accumulators of two row tiles
//   are the A fragment of the second product (contraction over rows, the same slot order), the coefficient p - [i == tgt] rounded to bf16; the
//   B fragments are prec_b gathered down the rows by dwords as above.  IT = 4 for a table of >= ITEMS_WIDE_TILES tiles, else 1 (a small table
//   has too few tiles to give every SIMD a wave otherwise).  Every table row is written by exactly one wave, once.
// No float atomics, a fixed schedule: the same inputs give the same bits.  Nothing of size rows x items is written.  E = 64 and 128: at 256 the
// backward's G x E output accumulators alone are 256 registers a lane beside the 128 of the row tiles.
#include "a4r_common.h"
#include "../../include/a4r.h"

namespace {

constexpr int MAX_RANGES = A4R_SCORE_CE_MAX_RANGES;
constexpr int G = A4R_SCORE_CE_BF16_ROWS;
constexpr int RT = G / 16;
constexpr int ITEMS_WIDE_TILES = 8192;      // 131 072 items: from here a wave of the item launch owns 4 tiles

A4R_DEV void lse_merge(float& m, float& l, float m2, float l2) {       // (as a4r_score_ce.hip: an empty set is (-inf, 0))
    const float mn = fmaxf(m, m2);
    const float a = m == mn ? l : l * __expf(m - mn);
    const float b = m2 == mn ? l2 : l2 * __expf(m2 - mn);
    m = mn;
    l = a + b;
}

A4R_DEV bool ce_trained(const float* __restrict__ log_mask, int tg, int r, int N1) { return log_mask[r] != 0.f && tg >= 1 && tg < N1; }

A4R_DEV float ce_gw(const float* __restrict__ loss_ws, float loss_scale, const float* __restrict__ loss_scale_dev) {
    const float cnt = loss_ws[2];
    return cnt > 0.f ? loss_scale * (loss_scale_dev ? loss_scale_dev[0] : 1.f) / cnt : 0.f;
}

// the 16-byte chunk (lane >> 4) of K step ks of a bf16 row
template <int E> A4R_DEV uint4 ld_chunk(const bf16_t* __restrict__ base, int row, int ks, int kg) {
    return *reinterpret_cast<const uint4*>(base + (size_t)row * E + ks * 32 + kg * 8);
}

// 8 dwords (one per contraction slot, each two neighbouring bf16 columns) -> the B fragments of the even and of the odd column
A4R_DEV uint4 frag_lo(const unsigned (&w)[8]) {
    return make_uint4((w[0] & 0xffffu) | (w[1] << 16), (w[2] & 0xffffu) | (w[3] << 16), (w[4] & 0xffffu) | (w[5] << 16), (w[6] & 0xffffu) | (w[7] << 16));
}
A4R_DEV uint4 frag_hi(const unsigned (&w)[8]) {
    return make_uint4((w[0] >> 16) | (w[1] & 0xffff0000u), (w[2] >> 16) | (w[3] & 0xffff0000u), (w[4] >> 16) | (w[5] & 0xffff0000u),
                      (w[6] >> 16) | (w[7] & 0xffff0000u));
}

// fp32 -> bf16, round to nearest even on the bit pattern (NaN stays a quiet NaN); integer work, so it does not depend on the denormal mode
A4R_DEV unsigned rne_bits(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ void __launch_bounds__(256) cast_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long n) {
    const long n8 = n >> 3;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < n8; c += (long)gridDim.x * 256) {
        const float4 a = *reinterpret_cast<const float4*>(src + c * 8), b = *reinterpret_cast<const float4*>(src + c * 8 + 4);
        *reinterpret_cast<uint4*>(dst + c * 8) = make_uint4(rne_bits(a.x) | (rne_bits(a.y) << 16), rne_bits(a.z) | (rne_bits(a.w) << 16),
                                                            rne_bits(b.x) | (rne_bits(b.y) << 16), rne_bits(b.z) | (rne_bits(b.w) << 16));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[n8 * 8 + threadIdx.x] = (unsigned short)rne_bits(src[n8 * 8 + threadIdx.x]);
}

template <int E>
__global__ void __launch_bounds__(256) ceb_fwd_kernel(const bf16_t* __restrict__ prec, const bf16_t* __restrict__ table,
                                                      const int32_t* __restrict__ tgt, float* __restrict__ ws, int R, int N1) {
    constexpr int KS = E / 32;
    __shared__ float red[4][G][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int r0 = blockIdx.x * G;
    uint4 ua[RT][KS];
    int tg[RT][4];
    float m[RT][4], l[RT][4], st[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int urow = min(r0 + rt * 16 + r16, R - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ua[rt][ks] = ld_chunk<E>(prec, urow, ks, kg);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = r0 + rt * 16 + kg * 4 + rr;
            tg[rt][rr] = row < R ? tgt[row] : 0;
            m[rt][rr] = -__builtin_huge_valf(); l[rt][rr] = 0.f; st[rt][rr] = 0.f;
        }
    }
    const int ntiles = (N1 - 1 + 15) / 16, tstep = gridDim.y * 4;
    int t = blockIdx.y * 4 + wave;
    uint4 bn[KS];
    {
        const int irow = min(1 + min(t, ntiles - 1) * 16 + r16, N1 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[ks] = ld_chunk<E>(table, irow, ks, kg);
    }
    for (; t < ntiles; t += tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column
        uint4 b[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = bn[ks];
        const int irow = min(1 + min(t + tstep, ntiles - 1) * 16 + r16, N1 - 1);          // (past the end: the last tile again, never used)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[ks] = ld_chunk<E>(table, irow, ks, kg);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) Mma<bf16_t>::mma(ua[rt][ks], b[ks], acc);
            if (i < N1) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const float s = acc[rr], d = s - m[rt][rr];         // one exp per score, as ce_fwd_kernel
                    const float e = __expf(-fabsf(d));
                    if (d > 0.f) { l[rt][rr] = l[rt][rr] * e + 1.f; m[rt][rr] = s; } else l[rt][rr] += e;
                    if (i == tg[rt][rr]) st[rt][rr] = s;
                }
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {           // over the 16 item columns (the target's score sits in one lane: the others add 0)
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
    if (tid < G && r0 + tid < R) {
        float mm = red[0][tid][0], ll = red[0][tid][1], ss = red[0][tid][2];
#pragma unroll
        for (int w = 1; w < 4; ++w) { lse_merge(mm, ll, red[w][tid][0], red[w][tid][1]); ss += red[w][tid][2]; }
        float* o = ws + ((size_t)blockIdx.y * R + r0 + tid) * 4;
        o[0] = mm; o[1] = ll; o[2] = ss;
    }
}

// one workgroup: the ranges of every row in range order -> lse, s_tgt; the trained rows counted, their losses summed in fp64 in a fixed order
__global__ void __launch_bounds__(256) ceb_merge_kernel(const float* __restrict__ ws, const int32_t* __restrict__ tgt,
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

template <int E>
__global__ void __launch_bounds__(256) ceb_bwd_rows_kernel(const bf16_t* __restrict__ prec, const bf16_t* __restrict__ table,
                                                           const float* __restrict__ lse, float* __restrict__ ws, int R, int N1) {
    constexpr int KS = E / 32, NT = E / 16, NQ = E / 32;
    extern __shared__ float dsh[];                   // [G][E]: the 4 waves' partial sums, added in wave order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int r0 = blockIdx.x * G;
    uint4 ua[RT][KS];
    float lse_r[RT];
    f32x4_t d[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int urow = min(r0 + rt * 16 + r16, R - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ua[rt][ks] = ld_chunk<E>(prec, urow, ks, kg);
        lse_r[rt] = lse[urow];
#pragma unroll
        for (int n = 0; n < NT; ++n) d[rt][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const int npairs = (N1 - 1 + 31) / 32, ustep = gridDim.y * 4;
    int u = blockIdx.y * 4 + wave;
    uint4 bn[2][KS];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int irow = min(1 + min(u, npairs - 1) * 32 + h * 16 + r16, N1 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[h][ks] = ld_chunk<E>(table, irow, ks, kg);
    }
    for (; u < npairs; u += ustep) {
        uint4 b[2][KS];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[h][ks] = bn[h][ks];
            const int irow = min(1 + min(u + ustep, npairs - 1) * 32 + h * 16 + r16, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bn[h][ks] = ld_chunk<E>(table, irow, ks, kg);
        }
        const int i0 = 1 + u * 32 + kg * 4;             // slot j of this lane: item i0 + 16 (j >> 2) + (j & 3)
        uint4 pa[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};      // transposed tiles: a_h[rr] = s[row r16][item i0 + 16 h + rr]
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { Mma<bf16_t>::mma(b[0][ks], ua[rt][ks], a0); Mma<bf16_t>::mma(b[1][ks], ua[rt][ks], a1); }
            float p[8];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                p[rr] = i0 + rr < N1 ? __expf(a0[rr] - lse_r[rt]) : 0.f;
                p[4 + rr] = i0 + 16 + rr < N1 ? __expf(a1[rr] - lse_r[rt]) : 0.f;
            }
            pa[rt] = Elem<bf16_t>::pack(p);
        }
        const unsigned* grow[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            grow[j] = reinterpret_cast<const unsigned*>(table + (size_t)min(i0 + 16 * (j >> 2) + (j & 3), N1 - 1) * E) + r16;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            unsigned w[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = grow[j][q * 16];
            const uint4 lo = frag_lo(w), hi = frag_hi(w);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {           // d[rt][2 q + h][rr] = D[row 16 rt + 4 kg + rr][column 32 q + 2 r16 + h]
                Mma<bf16_t>::mma(pa[rt], lo, d[rt][2 * q]);
                Mma<bf16_t>::mma(pa[rt], hi, d[rt][2 * q + 1]);
            }
        }
    }
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        float* o = dsh + (rt * 16 + kg * 4 + rr) * E + (n >> 1) * 32 + 2 * r16 + (n & 1);
                        *o = w == 0 ? d[rt][n][rr] : *o + d[rt][n][rr];
                    }
        }
        __syncthreads();
    }
    for (int e = tid; e < G * E; e += 256) {
        const int row = r0 + e / E;
        if (row < R) ws[((size_t)blockIdx.y * R + row) * E + (e % E)] = dsh[e];
    }
}

// d_prec[r] = g w[r] (the ranges' partials in range order - table_b[tgt_r]); exact zeros for the rows that are not trained
__global__ void __launch_bounds__(256) ceb_rows_finish_kernel(const float* __restrict__ ws, const bf16_t* __restrict__ table,
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
            v = gw * (s - (float)table[(size_t)tg * E + e]);
        }
        d_prec[idx] = v;
    }
}

template <int E, int IT>
__global__ void __launch_bounds__(256) ceb_bwd_items_kernel(const bf16_t* __restrict__ prec, const bf16_t* __restrict__ table,
                                                            const int32_t* __restrict__ tgt, const float* __restrict__ log_mask,
                                                            const float* __restrict__ lse, const float* __restrict__ loss_ws, float loss_scale,
                                                            const float* __restrict__ loss_scale_dev, float* __restrict__ d_table, int ldg, int R,
                                                            int N1) {
    constexpr int KS = E / 32, NT = E / 16, NQ = E / 32;
    const float gw = ce_gw(loss_ws, loss_scale, loss_scale_dev);
    if (gw == 0.f) return;                               // no trained row (or a zero incoming gradient): the destination keeps its bits
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int ntiles = (N1 - 1 + 15) / 16, ngroups = (ntiles + IT - 1) / IT, rpairs = (R + 31) / 32;
    for (int grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
        uint4 b[IT][KS];
        f32x4_t d[IT][NT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int irow = min(1 + (grp * IT + it) * 16 + r16, N1 - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[it][ks] = ld_chunk<E>(table, irow, ks, kg);
#pragma unroll
            for (int n = 0; n < NT; ++n) d[it][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        uint4 an[2][KS];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int urow = min(h * 16 + r16, R - 1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) an[h][ks] = ld_chunk<E>(prec, urow, ks, kg);
        }
        for (int rp = 0; rp < rpairs; ++rp) {
            uint4 ua[2][KS];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ua[h][ks] = an[h][ks];
                const int urow = min(min(rp + 1, rpairs - 1) * 32 + h * 16 + r16, R - 1);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) an[h][ks] = ld_chunk<E>(prec, urow, ks, kg);
            }
            const int q0 = rp * 32 + kg * 4;             // slot j of this lane: row q0 + 16 (j >> 2) + (j & 3)
            int tgj[8];
            float lsej[8];                               // +inf where the row is not trained: exp(s - inf) = 0
            const unsigned* arow[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int row = q0 + 16 * (j >> 2) + (j & 3), rc = min(row, R - 1);
                const int tg = tgt[rc];
                const bool on = row < R && ce_trained(log_mask, tg, rc, N1);
                tgj[j] = on ? tg : -1;
                lsej[j] = on ? lse[rc] : __builtin_huge_valf();
                arow[j] = reinterpret_cast<const unsigned*>(prec + (size_t)rc * E) + r16;
            }
            uint4 bf[NT];                                // prec_b down the rows: tile n' = 2 q + h holds the columns 32 q + 2 r16 + h
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                unsigned w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = arow[j][q * 16];
                bf[2 * q] = frag_lo(w);
                bf[2 * q + 1] = frag_hi(w);
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int i = 1 + (grp * IT + it) * 16 + r16;           // this lane's item column of the score tiles
                f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};      // a_h[rr] = s[row q0 + 16 h + rr][item i]
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) { Mma<bf16_t>::mma(ua[0][ks], b[it][ks], a0); Mma<bf16_t>::mma(ua[1][ks], b[it][ks], a1); }
                float c[8];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    c[rr] = __expf(a0[rr] - lsej[rr]) - (i == tgj[rr] ? 1.f : 0.f);
                    c[4 + rr] = __expf(a1[rr] - lsej[4 + rr]) - (i == tgj[4 + rr] ? 1.f : 0.f);
                }
                const uint4 ca = Elem<bf16_t>::pack(c);
#pragma unroll
                for (int n = 0; n < NT; ++n) Mma<bf16_t>::mma(ca, bf[n], d[it][n]);      // d[it][n][rr] = G[item 4 kg + rr of the tile][column of tile n]
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int item = 1 + (grp * IT + it) * 16 + kg * 4 + rr;
                if (item < N1) {
                    float* o = d_table + (size_t)item * ldg + 2 * r16;
#pragma unroll
                    for (int n = 0; n < NT; ++n) o[(n >> 1) * 32 + (n & 1)] += gw * d[it][n][rr];
                }
            }
    }
}

bool ceb_width_ok(int E) { return E == 64 || E == 128; }
bool ceb_shape_ok(int R, int N1, int E, int ranges) { return R > 0 && N1 >= 2 && ceb_width_ok(E) && ranges >= 0 && ranges <= MAX_RANGES; }

// the library's range count: about two workgroups per CU over the 64-row groups, at most MAX_RANGES and at most one range per 16-item tile
int ceb_ranges(int R, int N1) {
    const int gx = (R + G - 1) / G, ntiles = (N1 - 1 + 15) / 16;
    int gy = (2 * a4r_cu_count() + gx - 1) / gx;
    if (gy > MAX_RANGES) gy = MAX_RANGES;
    if (gy > ntiles) gy = ntiles;
    return gy < 1 ? 1 : gy;
}

template <int E> int launch_rows(hipStream_t s, dim3 grid, const bf16_t* prec, const bf16_t* table, const float* lse, float* ws, int R, int N1) {
    const size_t lds = (size_t)G * E * sizeof(float);
    if (int rc = a4r_set_lds(ceb_bwd_rows_kernel<E>, lds)) return rc;
    hipLaunchKernelGGL((ceb_bwd_rows_kernel<E>), grid, dim3(256), lds, s, prec, table, lse, ws, R, N1);
    return A4R_OK;
}
template <int E, int IT>
void launch_items(hipStream_t s, int ntiles, const bf16_t* prec, const bf16_t* table, const int32_t* tgt, const float* log_mask, const float* lse,
                  const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table, int ldg, int R, int N1) {
    const int ngroups = (ntiles + IT - 1) / IT, cap = 8 * a4r_cu_count();
    int grid = (ngroups + 3) / 4;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL((ceb_bwd_items_kernel<E, IT>), dim3(grid), dim3(256), 0, s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale,
                       loss_scale_dev, d_table, ldg, R, N1);
}
template <int E>
void launch_items_e(hipStream_t s, const bf16_t* prec, const bf16_t* table, const int32_t* tgt, const float* log_mask, const float* lse,
                    const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table, int ldg, int R, int N1) {
    const int ntiles = (N1 - 1 + 15) / 16;
    if (ntiles >= ITEMS_WIDE_TILES) launch_items<E, 4>(s, ntiles, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    else launch_items<E, 1>(s, ntiles, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
}

bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

}  // namespace

extern "C" int a4r_score_ce_bf16_cast(void* stream, const float* src, void* dst, int64_t n) {
    if (!src || !dst || n <= 0 || !aligned16(src, dst)) return A4R_EINVAL;
    const int64_t chunks = (n + 7) / 8, blocks = (chunks + 255) / 256;
    hipLaunchKernelGGL(cast_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
                       static_cast<unsigned short*>(dst), (long)n);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bf16_ranges(int R, int N1) {
    if (R <= 0 || N1 < 2) return A4R_EINVAL;
    return ceb_ranges(R, N1);
}

extern "C" size_t a4r_score_ce_bf16_ws_bytes(int R, int N1, int E, int ranges) {
    if (!ceb_shape_ok(R, N1, E, ranges)) return 0;
    const int gy = ranges ? ranges : ceb_ranges(R, N1);
    return (size_t)gy * (size_t)R * (size_t)E * sizeof(float);          // the backward's partials; the forward's triples (4 floats a row) fit in it
}

extern "C" int a4r_score_ce_bf16_fwd(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask, float* lse,
                                     float* s_tgt, float* loss_ws, void* ws, int R, int N1, int E, int ranges) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !s_tgt || !loss_ws || !ws || !ceb_shape_ok(R, N1, E, ranges)) return A4R_EINVAL;
    if (!aligned16(prec_b, table_b) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    const int gy = ranges ? ranges : ceb_ranges(R, N1);
    const dim3 grid((R + G - 1) / G, gy);
    float* w = static_cast<float*>(ws);
    if (E == 64) hipLaunchKernelGGL(ceb_fwd_kernel<64>, grid, dim3(256), 0, s, prec, table, tgt, w, R, N1);
    else hipLaunchKernelGGL(ceb_fwd_kernel<128>, grid, dim3(256), 0, s, prec, table, tgt, w, R, N1);
    hipLaunchKernelGGL(ceb_merge_kernel, dim3(1), dim3(256), 0, s, w, tgt, log_mask, lse, s_tgt, loss_ws, R, N1, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bf16_bwd_rows(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                                          const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_prec,
                                          void* ws, int R, int N1, int E, int ranges) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !loss_ws || !d_prec || !ws || !ceb_shape_ok(R, N1, E, ranges)) return A4R_EINVAL;
    if (!aligned16(prec_b, table_b) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    const int gy = ranges ? ranges : ceb_ranges(R, N1);
    const dim3 grid((R + G - 1) / G, gy);
    float* w = static_cast<float*>(ws);
    const int rc = E == 64 ? launch_rows<64>(s, grid, prec, table, lse, w, R, N1) : launch_rows<128>(s, grid, prec, table, lse, w, R, N1);
    if (rc) return rc;
    const size_t total = (size_t)R * E;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(ceb_rows_finish_kernel, dim3(blocks), dim3(256), 0, s, w, table, tgt, log_mask, loss_ws, loss_scale, loss_scale_dev, d_prec,
                       R, N1, E, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bf16_bwd_items(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                                           const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table,
                                           int ldg, int R, int N1, int E) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !loss_ws || !d_table || !ceb_shape_ok(R, N1, E, 0) || ldg < E) return A4R_EINVAL;
    if (!aligned16(prec_b, table_b)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    if (E == 64) launch_items_e<64>(s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    else launch_items_e<128>(s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    return a4r_launch_status();
}
