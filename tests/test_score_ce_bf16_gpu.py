"""GPU: the bf16 cross-entropy head's kernels (csrc/a4r_score_ce_bf16.hip: a4r_score_ce_bf16_cast, _fwd, _bwd_rows, _bwd_items) against the fp64
restatement at the bf16-rounded operands (tests/score_ce_bf16_ref.py) at the smallest shapes where they can go wrong: rows around the 16-row
tile and the 64-row group, items around the 16-item tile and the 32-item contraction pair, one to five item ranges (more ranges than tiles
included), both widths, and the item launch's wide path (>= 8192 item tiles, 4 tiles a wave).  Inputs are those of test_score_ce_gpu.py::make_case;
the operands reach the kernels through the cast launch.  Bounds: lse and target score 2e-4 absolute, loss 1e-5 absolute (the operands are rounded
in the reference, so the forward keeps the fp32 head's bounds); both gradients element-wise inside score_ce_bf16_ref.bounds (2^-8 of the summed
coefficient magnitudes: derived there, under 1 % of the gradients' size).

Measured worst errors on an MI355X (printed by the tests; d_prec / d_table as the worst error / bound ratio over the elements, loss scale 0.37 as a
host scalar, then as a device scalar):
    R=1 N=1 E=64 ranges=1 lse=5.96e-08 s_tgt=5.96e-08 loss=0.00e+00 d_prec=0.000 d_table=0.000 d_prec=0.000 d_table=0.000
    R=1 N=1 E=128 ranges=5 lse=3.35e-07 s_tgt=3.35e-07 loss=0.00e+00 d_prec=0.000 d_table=0.000 d_prec=0.000 d_table=0.000
    R=15 N=15 E=64 ranges=2 lse=2.77e-07 s_tgt=7.45e-08 loss=2.41e-08 d_prec=0.447 d_table=0.576 d_prec=0.447 d_table=0.576
    R=16 N=16 E=128 ranges=1 lse=4.07e-07 s_tgt=8.94e-08 loss=1.08e-07 d_prec=0.428 d_table=0.591 d_prec=0.428 d_table=0.591
    R=17 N=17 E=64 ranges=3 lse=2.38e-07 s_tgt=1.19e-07 loss=1.88e-07 d_prec=0.433 d_table=0.442 d_prec=0.433 d_table=0.442
    R=33 N=31 E=64 ranges=5 lse=3.10e-07 s_tgt=1.42e-07 loss=3.45e-08 d_prec=0.373 d_table=0.568 d_prec=0.373 d_table=0.568
    R=33 N=100 E=128 ranges=1 lse=5.68e-07 s_tgt=1.19e-07 loss=1.57e-07 d_prec=0.232 d_table=0.473 d_prec=0.232 d_table=0.473
    R=63 N=32 E=64 ranges=2 lse=5.37e-07 s_tgt=1.19e-07 loss=8.98e-08 d_prec=0.350 d_table=0.343 d_prec=0.350 d_table=0.343
    R=64 N=33 E=128 ranges=2 lse=3.43e-07 s_tgt=1.77e-07 loss=1.16e-07 d_prec=0.372 d_table=0.418 d_prec=0.372 d_table=0.418
    R=65 N=100 E=64 ranges=3 lse=5.14e-07 s_tgt=1.45e-07 loss=3.24e-08 d_prec=0.235 d_table=0.427 d_prec=0.235 d_table=0.427
    R=129 N=257 E=64 ranges=5 lse=7.00e-07 s_tgt=2.68e-07 loss=1.06e-07 d_prec=0.145 d_table=0.430 d_prec=0.145 d_table=0.430
    R=129 N=257 E=128 ranges=2 lse=6.98e-07 s_tgt=2.83e-07 loss=1.68e-07 d_prec=0.177 d_table=0.429 d_prec=0.177 d_table=0.429
    R=16 N=32 E=128 ranges=3 lse=5.61e-07 s_tgt=2.24e-07 loss=9.42e-08 d_prec=0.355 d_table=0.545 d_prec=0.355 d_table=0.545
    R=64 N=257 E=64 ranges=1 lse=6.75e-07 s_tgt=1.19e-07 loss=4.46e-08 d_prec=0.143 d_table=0.466 d_prec=0.143 d_table=0.466
    R=65 N=31 E=128 ranges=5 lse=3.76e-07 s_tgt=2.68e-07 loss=1.46e-07 d_prec=0.400 d_table=0.363 d_prec=0.400 d_table=0.363
    R=63 N=100 E=128 ranges=1 lse=4.82e-07 s_tgt=2.07e-07 loss=1.36e-07 d_prec=0.386 d_table=0.618 d_prec=0.386 d_table=0.618
    R=15 N=33 E=64 ranges=1 lse=4.80e-07 s_tgt=1.02e-07 loss=1.60e-07 d_prec=0.389 d_table=0.672 d_prec=0.389 d_table=0.672
    R=17 N=15 E=128 ranges=2 lse=2.68e-07 s_tgt=1.01e-07 loss=2.56e-08 d_prec=0.488 d_table=0.594 d_prec=0.488 d_table=0.594
    R=33 N=131100 E=64 ranges=0 lse=1.22e-06 s_tgt=1.79e-07 loss=7.47e-08 d_prec=0.008 d_table=0.063 d_prec=0.008 d_table=0.063
    R=17 N=131100 E=128 ranges=5 lse=1.52e-06 s_tgt=1.01e-07 loss=8.95e-07 d_prec=0.006 d_table=0.048 d_prec=0.006 d_table=0.048
    R=1280 N=14720 E=64 ranges=0 lse=1.51e-06 s_tgt=3.58e-07 loss=1.60e-07 d_prec=0.011 d_table=0.118 d_prec=0.011 d_table=0.118
    R=33 N=100 E=64 ranges=1 lse=1.13e-05 s_tgt=2.38e-06 loss=3.81e-07 d_prec=0.431 d_table=0.508 d_prec=0.431 d_table=0.508
    R=33 N=100 E=64 ranges=3 lse=1.13e-05 s_tgt=2.38e-06 loss=3.81e-07 d_prec=0.431 d_table=0.508 d_prec=0.431 d_table=0.508
The last two lines are the large-score case (prec x 28; its bound is 2e-4 x max |score|), the line before them the workload-sized head, the two
before that the item launch with four tiles a wave.
"""
import numpy as np
import pytest
import torch

import score_ce_bf16_ref as B16
import test_score_ce_gpu as G32

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALE = 0.37
_REF = {}


def reference(R, N, E, scale=1.0, mask='some'):
    key = (R, N, E, scale, mask)
    if key not in _REF:
        case = G32.make_case(R, N, E, scale, mask)
        _REF[key] = (case, B16.reference(*case))
    return _REF[key]


def to_dev(case):
    """(prec_b, table_b, tgt, mask) on the device: the two operands through the cast launch."""
    from adapter4rec_amd import _lib as L
    prec, table, tgt, m = [torch.from_numpy(a).to(DEV) for a in case]
    prec_b, table_b = torch.empty_like(prec, dtype=torch.bfloat16), torch.empty_like(table, dtype=torch.bfloat16)
    L.cast_bf16(prec, prec_b)
    L.cast_bf16(table, table_b)
    return prec_b, table_b, tgt, m


def bits16(t):
    return t.view(torch.int16).cpu().numpy().astype(np.uint16).astype(np.uint32)


def forward(dev_case, ranges):
    from adapter4rec_amd import _lib as L
    prec_b, table_b, tgt, m = dev_case
    R = prec_b.shape[0]
    nan = float('nan')
    lse, s_tgt, lw = torch.full((R,), nan, device=DEV), torch.full((R,), nan, device=DEV), torch.full((4,), nan, device=DEV)
    L.score_ce_bf16_fwd(prec_b, table_b, tgt, m, lse, s_tgt, lw, R, ranges=ranges)
    return lse, s_tgt, lw


def backward(dev_case, lse, lw, ranges, g0, host_scale=SCALE, scale_dev=None):
    from adapter4rec_amd import _lib as L
    prec_b, table_b, tgt, m = dev_case
    d_prec = torch.full(prec_b.shape, float('nan'), device=DEV)
    d_table = g0.clone()
    L.score_ce_bf16_bwd(prec_b, table_b, tgt, m, lse, lw, host_scale, d_prec, d_table, prec_b.shape[0], ranges=ranges, scale_dev=scale_dev)
    return d_prec, d_table


def check_case(R, N, E, ranges, scale=1.0, mask='some'):
    case, ref = reference(R, N, E, scale, mask)
    dev = to_dev(case)
    prec_b, table_b = B16.round_bf16(case[0]), B16.round_bf16(case[1])
    assert np.array_equal(bits16(dev[0]), prec_b.view(np.uint32) >> 16)          # the cast launch is the RNE of the reference
    assert np.array_equal(bits16(dev[1]), table_b.view(np.uint32) >> 16)
    lse, s_tgt, lw = forward(dev, ranges)
    torch.cuda.synchronize()
    f64 = lambda t: t.double().cpu().numpy()
    assert np.isfinite(f64(lse)).all() and np.isfinite(f64(s_tgt)).all() and np.isfinite(f64(lw)[:3]).all()
    e_lse, e_st = np.abs(f64(lse) - ref['lse']).max(), np.abs(f64(s_tgt) - ref['s_tgt']).max()
    e_loss = abs(float(lw[0]) - ref['loss'])
    fig = f'GPU ce bf16 R={R} N={N} E={E} ranges={ranges} lse={e_lse:.2e} s_tgt={e_st:.2e} loss={e_loss:.2e}'
    assert float(lw[2]) == ref['count'], fig
    g0_np = (np.random.default_rng(9).standard_normal((N + 1, E)) * 0.01).astype(np.float32)
    g0 = torch.from_numpy(g0_np).to(DEV)
    b_prec, b_table = B16.bounds(ref, prec_b, table_b, case[2], SCALE)
    want_p, want_t = ref['d_prec'] * SCALE, g0_np.astype(np.float64) + ref['d_table'] * SCALE
    errs = []
    for host, dev_scale in ((SCALE, None), (1.0, torch.tensor([SCALE], device=DEV))):
        d_prec, d_table = backward(dev, lse, lw, ranges, g0, host, dev_scale)
        dp, dt = f64(d_prec), f64(d_table)
        assert np.isfinite(dp).all() and np.isfinite(dt).all(), fig                     # (NaN = an element of d_prec the backward did not write)
        errs.append((np.abs(dp - want_p), np.abs(dt - want_t)))
        fig += f' d_prec={(errs[-1][0] / b_prec).max():.3f} d_table={(errs[-1][1] / b_table).max():.3f}'
        assert np.array_equal(d_table[0].cpu().numpy().view(np.uint32), g0_np[0].view(np.uint32)), fig        # row 0: bit-unchanged
        untrained = (case[3] == 0) | (case[2] == 0)
        assert not dp[untrained].any(), fig
    print(fig)
    if scale != 1.0:                                     # the large-score case: finite everywhere (asserted above), lse within 2e-4 x max |score|
        assert max(e_lse, e_st) <= 2e-4 * np.abs(ref['s']).max(), fig
        return ref, fig
    assert e_lse <= 2e-4 and e_st <= 2e-4, fig
    assert e_loss <= 1e-5, fig
    for ep, et in errs:
        assert np.all(ep <= b_prec), fig
        assert np.all(et <= b_table), fig
    return ref, fig


@pytest.mark.parametrize('R,N,E,ranges', B16.SHAPES)
def test_kernels_vs_fp64(R, N, E, ranges):
    """Forward (lse, target score, loss, trained-row count) and both backward launches, loss scale 0.37 as a host and as a device scalar, d_table
    accumulated onto a non-zero destination whose row 0 keeps its bits, exact zeros in d_prec on untrained rows."""
    ref, _ = check_case(R, N, E, ranges)
    assert ref['count'] > 0


@pytest.mark.parametrize('R,N,E,ranges', B16.WIDE_SHAPES)
def test_item_launch_with_four_tiles_a_wave(R, N, E, ranges):
    """A table of >= 8192 item tiles: a wave of the item launch owns four tiles (the last group here holds two, the last of them partial)."""
    assert (N + 15) // 16 >= 8192 and ((N + 15) // 16) % 4 and N % 16
    check_case(R, N, E, ranges)


def test_workload_head_size():
    """The flagship head: 64 users x 20 positions against 14 720 items, E = 64, the library's own range count."""
    check_case(*B16.WORKLOAD)


@pytest.mark.parametrize('R,N,E,ranges', B16.OTHER_SHAPES[:2])
def test_all_rows_masked(R, N, E, ranges):
    """No trained row: loss 0, d_prec exactly 0 everywhere, d_table's destination bit-unchanged, nothing non-finite."""
    case, ref = reference(R, N, E, 1.0, 'all')
    assert ref['count'] == 0
    dev = to_dev(case)
    lse, s_tgt, lw = forward(dev, ranges)
    assert float(lw[0]) == 0.0 and float(lw[2]) == 0.0 and bool(torch.isfinite(lse).all())
    assert np.abs(lse.double().cpu().numpy() - ref['lse']).max() <= 2e-4
    for g0 in (torch.zeros(N + 1, E, device=DEV), torch.randn(N + 1, E, device=DEV)):
        d_prec, d_table = backward(dev, lse, lw, ranges, g0)
        assert float(d_prec.abs().max()) == 0.0 and not bool(torch.isnan(d_prec).any())
        assert torch.equal(d_table.view(torch.int32), g0.view(torch.int32))


def test_zero_incoming_gradient_writes_nothing():
    """g == 0 (a device scalar of 0): d_prec exact zeros, the destination of d_table keeps its bits."""
    case, ref = reference(33, 100, 64)
    dev = to_dev(case)
    lse, s_tgt, lw = forward(dev, 2)
    g0 = torch.randn(101, 64, device=DEV)
    d_prec, d_table = backward(dev, lse, lw, 2, g0, 1.0, torch.zeros(1, device=DEV))
    assert ref['count'] > 0 and float(d_prec.abs().max()) == 0.0
    assert torch.equal(d_table.view(torch.int32), g0.view(torch.int32))


@pytest.mark.parametrize('ranges', [1, 3])
def test_large_scores_stay_finite(ranges):
    """prec scaled so that the scores reach about +-100: without max subtraction exp overflows.  Everything finite; lse (and the target score) within
    2e-4 x max |score|."""
    ref, fig = check_case(33, 100, 64, ranges, scale=28.0)
    assert 80 <= np.abs(ref['s']).max() <= 140, np.abs(ref['s']).max()


@pytest.mark.parametrize('ranges', [1, 5])
def test_two_calls_give_the_same_bits(ranges):
    case, _ = reference(33, 100, 64)
    g0 = torch.randn(101, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = []
    for _ in range(2):
        dev = to_dev(case)
        lse, s_tgt, lw = forward(dev, ranges)
        d_prec, d_table = backward(dev, lse, lw, ranges, g0)
        outs.append([t.clone() for t in (lw[:3], lse, s_tgt, d_prec, d_table)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(outs[0][4], g0)


BAD = [dict(E=96), dict(E=32), dict(E=256), dict(R=0), dict(R=-3), dict(N1=1), dict(ranges=33), dict(ranges=-1), dict(shift='prec'), dict(shift='table')]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '_'.join(f'{k}{v}' for k, v in b.items()))
def test_invalid_arguments_are_refused_before_any_launch(bad):
    """An unserved width, R <= 0, N1 < 2, ranges outside 0 .. 32, an operand that is not 16-byte aligned: the library's invalid-argument status
    from every entry point that takes the argument, and every output keeps its fill."""
    from adapter4rec_amd import _lib as L
    E, N1, R, ranges = bad.get('E', 64), bad.get('N1', 40), bad.get('R', 16), bad.get('ranges', 1)
    if E in L.SCORE_CE_BF16_E and 'E' in bad:
        pytest.fail(f'width {E} is served: not a refusal case')

    def operand(rows, shifted):                          # a contiguous bf16 [rows, E] view, 2 bytes off a 16-byte boundary when shifted
        flat = torch.zeros(rows * E + 8, dtype=torch.bfloat16, device=DEV)
        return flat[1:1 + rows * E].view(rows, E) if shifted else flat[:rows * E].view(rows, E)

    prec_b, table_b = operand(16, bad.get('shift') == 'prec'), operand(N1, bad.get('shift') == 'table')
    assert (prec_b.data_ptr() % 16 != 0) == (bad.get('shift') == 'prec') and (table_b.data_ptr() % 16 != 0) == (bad.get('shift') == 'table')
    tgt, m = torch.ones(16, dtype=torch.int32, device=DEV), torch.ones(16, device=DEV)
    outs = [torch.full(s, 7.0, device=DEV) for s in ((16,), (16,), (4,), (16, E), (N1, E))]
    lse, s_tgt, lw, d_prec, d_table = outs
    status = r'status -1 \(invalid argument\)'
    with pytest.raises(RuntimeError, match=status):
        L.score_ce_bf16_fwd(prec_b, table_b, tgt, m, lse, s_tgt, lw, R, ranges=ranges)
    with pytest.raises(RuntimeError, match=status):
        L.score_ce_bf16_bwd(prec_b, table_b, tgt, m, lse, lw, 1.0, d_prec, None, R, ranges=ranges)
    if 'ranges' not in bad:                              # (the item launch has no ranges: a wave owns whole item tiles)
        with pytest.raises(RuntimeError, match=status):
            L.score_ce_bf16_bwd(prec_b, table_b, tgt, m, lse, lw, 1.0, None, d_table, R)
    torch.cuda.synchronize()
    for t in outs:
        assert float((t - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize('n', [1, 7, 8, 9, 255, 256, 257, 16 * 64 + 3])
def test_cast_launch_is_round_to_nearest_even(n):
    """a4r_score_ce_bf16_cast against round_bf16 bit for bit around its 8-element chunks; the elements behind n keep their fill.  Values: random
    over many binades, exact ties after an even and an odd kept bit, denormals, +-inf, +-0."""
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    special = np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x00000001, 0x00018000, 0x807fffff, 0x7f800000, 0xff800000, 0x80000000,
                        0x7f7fffff], np.uint32).view(np.float32)
    k = min(n, len(special))
    x[n - k:] = special[:k]
    src = torch.from_numpy(x).to(DEV)
    dst = torch.full((n + 8,), 3.0, dtype=torch.bfloat16, device=DEV)
    L.cast_bf16(src, dst, n)
    got = bits16(dst)
    assert np.array_equal(got[:n], B16.round_bf16(x).view(np.uint32) >> 16)
    assert np.all(got[n:] == 0x4040)                     # (3.0)
    with pytest.raises(RuntimeError, match=r'status -1 \(invalid argument\)'):
        L.cast_bf16(src, dst, 0)
