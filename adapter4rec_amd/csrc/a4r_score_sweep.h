// The item-table score sweep: the one way this library forms score(r, i) = <rows[r], table[i]> for every item i = 1 .. N1-1 (row 0 of the table
// is the pad row: never a candidate) without materialising [rows, items].  Its users: eval_rank_kernel (a4r_eval.hip), topk_partial_kernel
// (a4r_topk.hip), the fp32 CE head (a4r_score_ce.hip) and the bf16 CE head (a4r_score_ce_bf16.hip).
//
//   Fragments.  16 rows of an operand are one MFMA fragment set: lane (r16 = lane & 15, kg = lane >> 4) holds, for K step ks, the 16-byte chunk
//     ks * 4 + kg of row r16 -- 16 / sizeof(T) elements, so a row of E elements is KS = E / (64 / sizeof(T)) steps (frag_load).  The rows of a
//     workgroup are loaded once and stay in registers.
//   Score tile.  KS Mma<T> steps into a zeroed accumulator (score_tile): acc[rr] = score(A row 4 kg + rr, B row r16).  An element's bits depend on
//     the two rows only, not on the tile or the column it sits in -- which is what lets eval compare a streamed score with the target's, and a
//     test hold top-K against eval.  score_tile(b, a) is the transposed tile of the *_bwd_rows kernels.
//   Deal.  The table is cut into tiles of W = 16 items (32 for the item pairs of ceb_bwd_rows_kernel); range y of the gridDim.y item ranges owns
//     the tiles 4 y + wave + 4 gridDim.y k of its four waves (SweepDeal).  A lane column past the table reads row N1 - 1 and is masked by its user.
//   Request ahead.  The fragments of a wave's NEXT tile are requested before this tile's products (sweep_begin / sweep_next): the table comes
//     from L2 / the Infinity Cache at 500+ cycles a request, and with one tile in flight per wave eval ran at 0.23 of the fp32 MFMA rate --
//     waiting, not streaming (profiles/r06_e_eval_host.txt).  Past the end the last tile is requested again and never used.  PF = false is the
//     form without it, for the kernels whose registers go to something else; the launchers choose per width.
//
// Free functions over the kernel's own uint4[KS] arrays on purpose: an iterator object that carried the fragments cost eval_rank_kernel<512> 16
// registers and a wave per SIMD.  These loops are a few dozen instructions, and how hipcc orders their loads decides their speed, so a kernel
// moves onto a piece of this header only with a timing beside the parent's: eval_rank_kernel's hot loop and ceb_bwd_rows_kernel's loads write
// the same sweep out themselves, because through sweep_next they ran 9 % and 27 % slower with the same bits (profiles/LOG.md, "One home for
// the item-table score sweep").
#pragma once
#include "a4r_common.h"
#include <type_traits>
#include <utility>

namespace {      // every user gets its own copy; nothing here becomes an export of the library

template <int E, typename T, int KS> A4R_DEV void frag_load(uint4 (&f)[KS], const T* __restrict__ base, int row, int kg) {
    static_assert(KS * 64 == E * (int)sizeof(T), "a row is KS steps of four 16-byte chunks");
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) f[ks] = *reinterpret_cast<const uint4*>(base + (size_t)row * E + (ks * 4 + kg) * (16 / (int)sizeof(T)));
}
// One chunk of frag_load, for a kernel that keeps the loop over ks its own (ceb_bwd_rows_kernel).  Not frag_load's body: written through this
// function, ce_bwd_items_kernel<64> and <128> took 14 and 38 more registers and lost a wave per SIMD.
template <int E, typename T> A4R_DEV uint4 frag_chunk(const T* __restrict__ base, int row, int ks, int kg) {
    return *reinterpret_cast<const uint4*>(base + (size_t)row * E + (ks * 4 + kg) * (16 / (int)sizeof(T)));
}

template <typename T, int KS> A4R_DEV f32x4_t score_tile(const uint4 (&a)[KS], const uint4 (&b)[KS]) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) Mma<T>::mma(a[ks], b[ks], acc);
    return acc;
}

template <int W = 16> struct SweepDeal {
    const int N1, ntiles, tstep, first;              // first: this wave's first tile; a wave walks first, first + tstep, ... while < ntiles
    A4R_DEV SweepDeal(int N1_, int wave) : N1(N1_), ntiles((N1_ - 1 + W - 1) / W), tstep(gridDim.y * 4), first(blockIdx.y * 4 + wave) {}
    // steps of the workgroup's range, the same for its 4 waves (a wave's last tile may lie past the table): for a barrier at every step
    A4R_DEV int steps() const { const int f = blockIdx.y * 4; return f < ntiles ? (ntiles - f + tstep - 1) / tstep : 0; }
    // the table row of lane column col (< W) of tile t; a tile past the end is the last tile again
    A4R_DEV int row(int t, int col) const { return min(1 + min(t, ntiles - 1) * W + col, N1 - 1); }
};

// bn <- the fragments of the wave's first tile (PF only)
template <int E, bool PF, int W, typename T, int KN>
A4R_DEV void sweep_begin(uint4 (&bn)[KN], const T* __restrict__ table, const SweepDeal<W>& deal, int col, int kg) {
    if constexpr (PF) frag_load<E>(bn, table, deal.row(deal.first, col), kg);
}
// b <- the fragments of tile t.  PF: they are the ones requested a tile ago, and those of tile t + tstep are requested now
template <int E, bool PF, int W, typename T, int KS, int KN>
A4R_DEV void sweep_next(uint4 (&b)[KS], uint4 (&bn)[KN], const T* __restrict__ table, const SweepDeal<W>& deal, int t, int col, int kg) {
    if constexpr (PF) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[ks] = bn[ks];
        frag_load<E>(bn, table, deal.row(t + deal.tstep, col), kg);
    } else {
        frag_load<E>(b, table, deal.row(t, col), kg);
    }
}

// ---------------------------------------------------------------- host side
// The grid of eval and top-K: 16 rows per workgroup, about 2048 workgroups, at most one item range per 4 tiles (a tile per wave)
int sweep_ranges(int rows, int N1) {
    const int gx = (rows + 15) / 16, ntiles = (N1 - 1 + 15) / 16;
    int gy = 2048 / gx; if (gy < 1) gy = 1;
    return gy > (ntiles + 3) / 4 ? (ntiles + 3) / 4 : gy;
}

bool aligned16(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

// The widths a kernel family is instantiated for.  with_width calls f(std::integral_constant<int, E>{}) for the served width E -- the one place
// a run-time width becomes a template argument -- and says whether there was one.
template <int... Es> using Widths = std::integer_sequence<int, Es...>;
using WidthsF32 = Widths<64, 128, 256, 512>;
template <int... Es> bool width_served(Widths<Es...>, int E) { return ((E == Es) || ...); }
template <int... Es, typename F> bool with_width(Widths<Es...>, int E, F&& f) {
    return ((E == Es ? (f(std::integral_constant<int, Es>{}), true) : false) || ...);
}

}  // namespace
