"""What the bf16 cross-entropy head (include/a4r.h: a4r_score_ce_bf16_*) is held to: the fp64 restatement of tests/score_ce_ref.py evaluated at the
bf16-rounded operands, and the derived worst-case error of an implementation that rounds the probability (or coefficient) tile to bf16 as
the A operand of its second product.

    prec_b = bf16(prec), table_b = bf16(table)      (round to nearest even)
    reference(prec, table, tgt, mask) = score_ce_ref.reference(prec_b, table_b, tgt, mask)

The operands are rounded in the reference already, and the scores are accumulated in fp32 from exact products of bf16 numbers, so the forward
keeps the fp32 head's bounds (lse and s_tgt 2e-4 absolute, loss 1e-5).  The gradients: rounding one coefficient c to bf16 moves it by at most
2^-9 |c| (half an ulp of an 8-bit significand).  An implementation may round p and subtract the one-hot afterwards (error <= 2^-9 p) or round
p - [i == tgt] (error <= 2^-9 (p + [i == tgt]) as |p - 1| <= 1 + p); either is inside 2^-9 (p + [i == tgt]).  bounds() allows twice that,
2^-8, which leaves the other half for the fp32 accumulation and the exp of the kernels (each below 1e-6 relative), plus 1e-6 absolute:

    |err d_prec[r, e]|  <= 2^-8 g w[r] sum_i (p[r, i] + [i == tgt_r]) |table_b[i, e]| + 1e-6
    |err d_table[i, e]| <= 2^-8 g sum_r w[r] (p[r, i] + [i == tgt_r]) |prec_b[r, e]| + 1e-6

The factor is derived, not measured.  At every test input with more than one item the largest bound is 0.4 - 0.7 % of the largest gradient
element (tests/test_score_ce_bf16_cpu.py asserts under 1 %); a wrong item permutation or a dropped tile is an error of order 100 %.  The
N = 1 inputs are the exception: the one item has p = 1, every gradient is exactly 0, and the bound (2^-8 of 2 |operand| g w) is all there is."""
import numpy as np

import score_ce_ref as CE

G = 64                  # the rows a workgroup of the bf16 head holds (A4R_SCORE_CE_BF16_ROWS)
WIDE_ITEMS = 131100     # >= 8192 16-item tiles: the item launch's 4-tiles-a-wave path (csrc/a4r_score_ce_bf16.hip: ITEMS_WIDE_TILES), last group partial

# (R, N, E, ranges): R in {1, 15, 16, 17, 33, G-1, G, G+1, 2G+1} x N in {1, 15, 16, 17, 31, 32, 33, 100, 257} x ranges in {1, 2, 3, 5} x E in {64, 128}, a
# subset that holds every value of every dimension, more ranges than tiles (N <= 16 with ranges >= 2, N = 31 with ranges = 5), an odd number of
# 16-item tiles (N = 33, 100, 257: the 32-item contraction pair's second half empty or partial), and each E with each tile edge
SHAPES = [(1, 1, 64, 1), (1, 1, 128, 5), (15, 15, 64, 2), (16, 16, 128, 1), (17, 17, 64, 3), (33, 31, 64, 5), (33, 100, 128, 1), (63, 32, 64, 2),
          (64, 33, 128, 2), (65, 100, 64, 3), (129, 257, 64, 5), (129, 257, 128, 2), (16, 32, 128, 3), (64, 257, 64, 1), (65, 31, 128, 5),
          (63, 100, 128, 1), (15, 33, 64, 1), (17, 15, 128, 2)]
# the shapes of the further GPU tests: the item launch's wide path at both widths, the workload head, the masked / large-score / repeat cases
WIDE_SHAPES = [(33, WIDE_ITEMS, 64, 0), (17, WIDE_ITEMS, 128, 5)]
WORKLOAD = (1280, 14720, 64, 0)
OTHER_SHAPES = [(17, 33, 64, 1), (33, 100, 128, 5), (33, 100, 64, 1), (33, 100, 64, 3)]


def round_bf16(x):
    """fp32 -> the nearest bf16 (ties to even) as fp32, on the bit pattern: denormals are kept, +-inf stay, a NaN stays a NaN."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    r = np.where((u & 0x7fffffff) > 0x7f800000, (u | 0x400000) & 0xffff0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def reference(prec, table, tgt, log_mask):
    """score_ce_ref.reference at the rounded operands, plus w [R] (1 / count on trained rows) and p [R, N] for bounds()."""
    ref = CE.reference(round_bf16(prec), round_bf16(table), tgt, log_mask)
    trained = (np.asarray(log_mask).reshape(-1) != 0) & (np.asarray(tgt).reshape(-1) != 0)
    ref['w'] = trained / ref['count'] if ref['count'] else np.zeros(len(trained))
    ref['p'] = np.exp(ref['s'] - ref['lse'][:, None])
    return ref


def bounds(ref, prec_b, table_b, tgt, g):
    """-> (bound of |err d_prec| [R, E], bound of |err d_table| [N + 1, E]) for the incoming gradient g (the module docstring's two lines)."""
    tgt = np.asarray(tgt, np.int64).reshape(-1)
    a = ref['p'].copy()
    has = np.flatnonzero(tgt != 0)
    a[has, tgt[has] - 1] += 1.0
    a *= ref['w'][:, None]
    k = 2.0 ** -8 * abs(g)
    b_table = np.full(table_b.shape, 1e-6)
    b_table[1:] += k * (a.T @ np.abs(np.asarray(prec_b, np.float64)))
    return k * (a @ np.abs(np.asarray(table_b, np.float64)[1:])) + 1e-6, b_table
