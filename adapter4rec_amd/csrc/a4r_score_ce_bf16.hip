// The full-softmax cross-entropy head of the ID tower on the bf16 MFMA (--ce_dtype bf16): the function of a4r_score_ce.hip evaluated at
// prec_b = bf16(prec), table_b = bf16(table) (round to nearest even; a4r_score_ce_bf16_cast writes the two copies), scores accumulated in fp32.
//
//   s[r, i] = <prec_b[r], table_b[i]>, i = 1 .. N1-1;  lse, s_tgt, loss, count, trained(r), w[r] as a4r_score_ce_common.h states them
//   d_prec[r]  = g w[r] (sum_i p[r, i] table_b[i] - table_b[tgt_r])                 (straight-through: handed to the fp32 masters as it is)
//   d_table[i] += g sum_r w[r] (p[r, i] - [i == tgt_r]) prec_b[r]
//
// Why not the fp32 kernels with another Mma: at a large table they are bound by the bytes of a table pass as much as by the MFMA (every 16-row
// workgroup streams its whole item range).  Here a workgroup holds G = 64 rows -- each wave keeps the G / 16 = 4 row tiles of prec_b as A
// fragments (8 VGPRs a tile at E = 64) -- and a 16-item tile's B fragments, loaded once, meet all four: a quarter of the table passes at half
// the bytes a pass.  One v_mfma_f32_16x16x32_bf16 covers K = 32 (a lane's 16-byte chunk is 8 elements, k = 8 (lane >> 4) + j).
//
// Scores: the item-table score sweep of a4r_score_sweep.h at T = bf16_t.  Forward: the online update and the reduce-and-store of
// a4r_score_ce_common.h, four row tiles wide.  Range merge and the d_prec finish: the launches of that header.
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
#include "a4r_score_ce_common.h"

namespace {

constexpr int G = A4R_SCORE_CE_BF16_ROWS;
constexpr int RT = G / 16;
constexpr int ITEMS_WIDE_TILES = 8192;      // 131 072 items: from here a wave of the item launch owns 4 tiles

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
        frag_load<E>(ua[rt], prec, min(r0 + rt * 16 + r16, R - 1), kg);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int row = r0 + rt * 16 + kg * 4 + rr;
            tg[rt][rr] = row < R ? tgt[row] : 0;
            m[rt][rr] = -__builtin_huge_valf(); l[rt][rr] = 0.f; st[rt][rr] = 0.f;
        }
    }
    const SweepDeal<> deal(N1, wave);
    uint4 bn[KS];
    sweep_begin<E, true>(bn, table, deal, r16, kg);
    for (int t = deal.first; t < deal.ntiles; t += deal.tstep) {
        const int i = 1 + t * 16 + r16;                 // this lane's item column
        uint4 b[KS];
        sweep_next<E, true>(b, bn, table, deal, t, r16, kg);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const f32x4_t acc = score_tile<bf16_t>(ua[rt], b);
            if (i < N1) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) ce_online(acc[rr], i == tg[rt][rr], m[rt][rr], l[rt][rr], st[rt][rr]);
            }
        }
    }
    ce_reduce_store<G>(m, l, st, red, ws, R, r0);
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
        for (int ks = 0; ks < KS; ++ks) ua[rt][ks] = frag_chunk<E>(prec, urow, ks, kg);
        lse_r[rt] = lse[urow];
#pragma unroll
        for (int n = 0; n < NT; ++n) d[rt][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    // The sweep in pairs of 16-item tiles (lane column 16 h + r16 of pair u), chunk by chunk in this kernel's own loops: through frag_load /
    // sweep_next the compiler schedules the loop another way, and it ran 27 % slower at 500 000 items (profiles/LOG.md)
    const SweepDeal<32> deal(N1, wave);
    uint4 bn[2][KS];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int irow = deal.row(deal.first, h * 16 + r16);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bn[h][ks] = frag_chunk<E>(table, irow, ks, kg);
    }
    for (int u = deal.first; u < deal.ntiles; u += deal.tstep) {
        uint4 b[2][KS];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[h][ks] = bn[h][ks];
            const int irow = deal.row(u + deal.tstep, h * 16 + r16);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bn[h][ks] = frag_chunk<E>(table, irow, ks, kg);
        }
        const int i0 = 1 + u * 32 + kg * 4;             // slot j of this lane: item i0 + 16 (j >> 2) + (j & 3)
        uint4 pa[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            // transposed tiles: a_h[rr] = s[row r16][item i0 + 16 h + rr]
            const f32x4_t a0 = score_tile<bf16_t>(b[0], ua[rt]), a1 = score_tile<bf16_t>(b[1], ua[rt]);
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
    ce_rows_partial_store<G, E>(d, dsh, ws, R, r0, [](int n, int c) { return (n >> 1) * 32 + 2 * c + (n & 1); });
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
            frag_load<E>(b[it], table, min(1 + (grp * IT + it) * 16 + r16, N1 - 1), kg);
#pragma unroll
            for (int n = 0; n < NT; ++n) d[it][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        uint4 an[2][KS];
#pragma unroll
        for (int h = 0; h < 2; ++h) frag_load<E>(an[h], prec, min(h * 16 + r16, R - 1), kg);
        for (int rp = 0; rp < rpairs; ++rp) {
            uint4 ua[2][KS];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) ua[h][ks] = an[h][ks];
                frag_load<E>(an[h], prec, min(min(rp + 1, rpairs - 1) * 32 + h * 16 + r16, R - 1), kg);
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
                const f32x4_t a0 = score_tile<bf16_t>(ua[0], b[it]), a1 = score_tile<bf16_t>(ua[1], b[it]);      // a_h[rr] = s[row q0 + 16 h + rr][item i]
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

using WidthsBf16 = Widths<64, 128>;

template <int E, int IT>
void launch_items(hipStream_t s, int ntiles, const bf16_t* prec, const bf16_t* table, const int32_t* tgt, const float* log_mask, const float* lse,
                  const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table, int ldg, int R, int N1) {
    const int ngroups = (ntiles + IT - 1) / IT, cap = 8 * a4r_cu_count();
    int grid = (ngroups + 3) / 4;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL((ceb_bwd_items_kernel<E, IT>), dim3(grid), dim3(256), 0, s, prec, table, tgt, log_mask, lse, loss_ws, loss_scale,
                       loss_scale_dev, d_table, ldg, R, N1);
}

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
    return ce_ranges(R, N1, G);
}

extern "C" size_t a4r_score_ce_bf16_ws_bytes(int R, int N1, int E, int ranges) {
    if (!ce_shape_ok(WidthsBf16{}, R, N1, E, ranges)) return 0;
    return ce_ws_bytes(ranges ? ranges : ce_ranges(R, N1, G), R, E);
}

extern "C" int a4r_score_ce_bf16_fwd(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask, float* lse,
                                     float* s_tgt, float* loss_ws, void* ws, int R, int N1, int E, int ranges) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !s_tgt || !loss_ws || !ws) return A4R_EINVAL;
    if (!ce_args_ok(WidthsBf16{}, prec_b, table_b, R, N1, E, ranges) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    const int gy = ranges ? ranges : ce_ranges(R, N1, G);
    const dim3 grid((R + G - 1) / G, gy);
    float* w = static_cast<float*>(ws);
    with_width(WidthsBf16{}, E, [&](auto e) {
        hipLaunchKernelGGL(ceb_fwd_kernel<decltype(e)::value>, grid, dim3(256), 0, s, prec, table, tgt, w, R, N1);
    });
    hipLaunchKernelGGL(ce_merge_kernel, dim3(1), dim3(256), 0, s, w, tgt, log_mask, lse, s_tgt, loss_ws, R, N1, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bf16_bwd_rows(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                                          const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_prec,
                                          void* ws, int R, int N1, int E, int ranges) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !loss_ws || !d_prec || !ws) return A4R_EINVAL;
    if (!ce_args_ok(WidthsBf16{}, prec_b, table_b, R, N1, E, ranges) || (reinterpret_cast<uintptr_t>(ws) & 15u)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    const int gy = ranges ? ranges : ce_ranges(R, N1, G);
    const dim3 grid((R + G - 1) / G, gy);
    float* w = static_cast<float*>(ws);
    int rc = A4R_OK;
    with_width(WidthsBf16{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        const size_t lds = (size_t)G * W * sizeof(float);
        if ((rc = a4r_set_lds(ceb_bwd_rows_kernel<W>, lds))) return;
        hipLaunchKernelGGL(ceb_bwd_rows_kernel<W>, grid, dim3(256), lds, s, prec, table, lse, w, R, N1);
    });
    if (rc) return rc;
    launch_ce_rows_finish(s, w, table, tgt, log_mask, loss_ws, loss_scale, loss_scale_dev, d_prec, R, N1, E, gy);
    return a4r_launch_status();
}

extern "C" int a4r_score_ce_bf16_bwd_items(void* stream, const void* prec_b, const void* table_b, const int32_t* tgt, const float* log_mask,
                                           const float* lse, const float* loss_ws, float loss_scale, const float* loss_scale_dev, float* d_table,
                                           int ldg, int R, int N1, int E) {
    if (!prec_b || !table_b || !tgt || !log_mask || !lse || !loss_ws || !d_table || ldg < E) return A4R_EINVAL;
    if (!ce_args_ok(WidthsBf16{}, prec_b, table_b, R, N1, E, 0)) return A4R_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bf16_t* prec = static_cast<const bf16_t*>(prec_b);
    const bf16_t* table = static_cast<const bf16_t*>(table_b);
    const int ntiles = (N1 - 1 + 15) / 16;
    with_width(WidthsBf16{}, E, [&](auto e) {
        constexpr int W = decltype(e)::value;
        if (ntiles >= ITEMS_WIDE_TILES) launch_items<W, 4>(s, ntiles, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
        else launch_items<W, 1>(s, ntiles, prec, table, tgt, log_mask, lse, loss_ws, loss_scale, loss_scale_dev, d_table, ldg, R, N1);
    });
    return a4r_launch_status();
}
