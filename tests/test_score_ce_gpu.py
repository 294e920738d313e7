"""GPU: the cross-entropy head's kernels (csrc/a4r_score_ce.hip: a4r_score_ce_fwd, _bwd_rows, _bwd_items) against the fp64 restatement of
tests/score_ce_ref.py at the smallest shapes where they can go wrong: rows and items around the 16 x 16 tile, one to five item ranges (more
ranges than tiles included), every table width.  Inputs are scaled as in test_user_tower_kernels_gpu.py::test_head_vs_fp64 (E ** -0.25 each, unit
score variance).  Bounds (the ones that file holds the BCE head and the weight-gradient kernels to): lse and target score 2e-4 absolute, loss
1e-5 absolute, d_prec 1e-6 + 2e-4 |ref|, d_table 1e-4 max |ref| + 1e-6.

Measured worst errors on an MI355X (printed by the tests):
    R=1 N=1 E=64 ranges=1 lse=1.12e-07 s_tgt=1.12e-07 loss=0.00e+00 d_prec=0.00e+00 d_table=0.00e+00 d_prec=0.00e+00 d_table=0.00e+00
    R=1 N=1 E=64 ranges=5 lse=1.12e-07 s_tgt=1.12e-07 loss=0.00e+00 d_prec=0.00e+00 d_table=0.00e+00 d_prec=0.00e+00 d_table=0.00e+00
    R=15 N=15 E=64 ranges=2 lse=3.94e-07 s_tgt=2.99e-07 loss=4.86e-09 d_prec=5.75e-09 d_table=5.09e-09 d_prec=5.75e-09 d_table=5.09e-09
    R=16 N=16 E=64 ranges=1 lse=4.51e-07 s_tgt=4.92e-07 loss=1.21e-08 d_prec=5.25e-09 d_table=7.62e-09 d_prec=5.25e-09 d_table=7.62e-09
    R=17 N=17 E=64 ranges=3 lse=3.23e-07 s_tgt=2.63e-07 loss=2.32e-07 d_prec=3.35e-09 d_table=6.41e-09 d_prec=3.35e-09 d_table=6.41e-09
    R=33 N=31 E=64 ranges=5 lse=3.78e-07 s_tgt=3.48e-07 loss=2.94e-08 d_prec=3.07e-09 d_table=8.62e-09 d_prec=3.07e-09 d_table=8.62e-09
    R=33 N=100 E=64 ranges=1 lse=4.39e-07 s_tgt=8.52e-07 loss=5.72e-08 d_prec=2.12e-09 d_table=6.79e-09 d_prec=2.12e-09 d_table=6.79e-09
    R=16 N=33 E=64 ranges=2 lse=4.32e-07 s_tgt=2.86e-07 loss=1.96e-07 d_prec=7.09e-09 d_table=6.00e-09 d_prec=7.09e-09 d_table=6.00e-09
    R=33 N=33 E=128 ranges=2 lse=5.00e-07 s_tgt=9.19e-07 loss=1.23e-07 d_prec=3.13e-09 d_table=5.31e-09 d_prec=3.13e-09 d_table=5.31e-09
    R=15 N=100 E=128 ranges=3 lse=6.10e-07 s_tgt=4.65e-07 loss=2.71e-07 d_prec=4.66e-09 d_table=6.38e-09 d_prec=4.66e-09 d_table=6.38e-09
    R=1 N=17 E=128 ranges=5 lse=2.33e-07 s_tgt=7.27e-08 loss=3.06e-07 d_prec=2.38e-08 d_table=1.66e-08 d_prec=2.38e-08 d_table=1.66e-08
    R=17 N=100 E=256 ranges=3 lse=5.44e-07 s_tgt=5.62e-07 loss=1.07e-07 d_prec=4.35e-09 d_table=7.91e-09 d_prec=4.35e-09 d_table=7.91e-09
    R=33 N=17 E=256 ranges=5 lse=3.66e-07 s_tgt=6.88e-07 loss=1.76e-07 d_prec=3.16e-09 d_table=4.28e-09 d_prec=3.16e-09 d_table=4.28e-09
    R=15 N=31 E=256 ranges=1 lse=4.34e-07 s_tgt=9.58e-07 loss=1.13e-07 d_prec=8.28e-09 d_table=8.34e-09 d_prec=8.28e-09 d_table=8.34e-09
    R=16 N=100 E=512 ranges=5 lse=3.91e-07 s_tgt=6.70e-07 loss=1.19e-07 d_prec=9.53e-09 d_table=6.97e-09 d_prec=9.53e-09 d_table=6.97e-09
    R=17 N=16 E=512 ranges=2 lse=6.91e-07 s_tgt=6.66e-07 loss=1.44e-07 d_prec=4.19e-09 d_table=5.90e-09 d_prec=4.19e-09 d_table=5.90e-09
    R=33 N=15 E=512 ranges=1 lse=5.92e-07 s_tgt=1.17e-06 loss=1.14e-07 d_prec=5.00e-09 d_table=6.58e-09 d_prec=5.00e-09 d_table=6.58e-09
    R=1280 N=14720 E=64 ranges=0 lse=1.47e-06 s_tgt=9.08e-07 loss=1.85e-07 d_prec=1.14e-10 d_table=2.00e-09 d_prec=1.14e-10 d_table=2.00e-09
    R=33 N=100 E=64 ranges=1 lse=1.57e-05 s_tgt=1.33e-05 loss=1.36e-06 d_prec=6.61e-08 d_table=2.00e-06 d_prec=6.61e-08 d_table=2.00e-06
    R=33 N=100 E=64 ranges=3 lse=1.57e-05 s_tgt=1.33e-05 loss=1.36e-06 d_prec=6.59e-08 d_table=2.00e-06 d_prec=6.59e-08 d_table=2.00e-06
The last two lines are the large-score case (prec x 28, max |score| about 100; its bound is 2e-4 x max |score|), the line before them the
workload-sized head.  Each line holds d_prec / d_table twice: loss scale 0.37 as a host scalar, then as a device scalar.
"""
import numpy as np
import pytest
import torch

import score_ce_ref as CE

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALE = 0.37
_REF = {}


def make_case(R, N, E, scale=1.0, mask='some'):
    """Every case holds: a target in the last (partial) tile and equal to N (row 0), duplicate targets, rows with target 0, masked rows."""
    rng = np.random.default_rng([R, N, E])
    prec = (rng.standard_normal((R, E)) * E ** -0.25 * scale).astype(np.float32)
    table = (rng.standard_normal((N + 1, E)) * E ** -0.25).astype(np.float32)
    tgt = rng.integers(1, N + 1, R).astype(np.int32)
    m = np.ones(R, np.float32)
    tgt[0] = N
    if R > 4:
        tgt[1] = tgt[2] = N                          # duplicates of the last item
        tgt[3] = tgt[R - 1]                          # another duplicate pair
        tgt[4] = 0                                   # rows without a target
        tgt[R // 2] = 0
        if mask == 'some':
            m[5::3] = 0
    if mask == 'all':
        m[:] = 0
    return prec, table, tgt, m


def reference(R, N, E, scale=1.0, mask='some'):
    key = (R, N, E, scale, mask)
    if key not in _REF:
        case = make_case(R, N, E, scale, mask)
        _REF[key] = (case, CE.reference(*case))
    return _REF[key]


def to_dev(case):
    return [torch.from_numpy(a).to(DEV) for a in case]


def forward(dev_case, ranges):
    from adapter4rec_amd import _lib as L
    prec, table, tgt, m = dev_case
    R = prec.shape[0]
    nan = float('nan')
    lse, s_tgt, lw = torch.full((R,), nan, device=DEV), torch.full((R,), nan, device=DEV), torch.full((4,), nan, device=DEV)
    L.score_ce_fwd(prec, table, tgt, m, lse, s_tgt, lw, R, ranges=ranges)
    return lse, s_tgt, lw


def backward(dev_case, lse, lw, ranges, g0, host_scale=SCALE, scale_dev=None):
    from adapter4rec_amd import _lib as L
    prec, table, tgt, m = dev_case
    d_prec = torch.full_like(prec, float('nan'))
    d_table = g0.clone()
    L.score_ce_bwd(prec, table, tgt, m, lse, lw, host_scale, d_prec, d_table, prec.shape[0], ranges=ranges, scale_dev=scale_dev)
    return d_prec, d_table


def check_case(R, N, E, ranges, scale=1.0, mask='some'):
    case, ref = reference(R, N, E, scale, mask)
    dev = to_dev(case)
    lse, s_tgt, lw = forward(dev, ranges)
    torch.cuda.synchronize()
    f64 = lambda t: t.double().cpu().numpy()
    assert np.isfinite(f64(lse)).all() and np.isfinite(f64(s_tgt)).all() and np.isfinite(f64(lw)[:3]).all()
    e_lse, e_st = np.abs(f64(lse) - ref['lse']).max(), np.abs(f64(s_tgt) - ref['s_tgt']).max()
    e_loss = abs(float(lw[0]) - ref['loss'])
    fig = f'GPU ce R={R} N={N} E={E} ranges={ranges} lse={e_lse:.2e} s_tgt={e_st:.2e} loss={e_loss:.2e}'
    assert float(lw[2]) == ref['count'], fig
    g0_np = (np.random.default_rng(9).standard_normal((N + 1, E)) * 0.01).astype(np.float32)
    g0 = torch.from_numpy(g0_np).to(DEV)
    errs = []
    for host, dev_scale in ((SCALE, None), (1.0, torch.tensor([SCALE], device=DEV))):
        d_prec, d_table = backward(dev, lse, lw, ranges, g0, host, dev_scale)
        dp, dt = f64(d_prec), f64(d_table)
        assert np.isfinite(dp).all() and np.isfinite(dt).all(), fig                     # (NaN = an element of d_prec the backward did not write)
        want_p, want_t = ref['d_prec'] * SCALE, ref['d_table'] * SCALE
        errs.append((np.abs(dp - want_p), np.abs(dt - (g0_np.astype(np.float64) + want_t))))
        fig += f' d_prec={errs[-1][0].max():.2e} d_table={errs[-1][1].max():.2e}'
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
        assert np.all(ep <= 1e-6 + 2e-4 * np.abs(ref['d_prec'] * SCALE)), fig
        assert et.max() <= 1e-4 * np.abs(ref['d_table'] * SCALE).max() + 1e-6, fig
    return ref, fig


# R in {1, 15, 16, 17, 33} x N in {1, 15, 16, 17, 31, 33, 100} x ranges in {1, 2, 3, 5} x E in {64, 128, 256, 512}: a subset that holds every
# value of every dimension, more ranges than tiles (N <= 16 with ranges >= 2, N = 31 / 33 with ranges = 5), and each E with each tile edge
SHAPES = [(1, 1, 64, 1), (1, 1, 64, 5), (15, 15, 64, 2), (16, 16, 64, 1), (17, 17, 64, 3), (33, 31, 64, 5), (33, 100, 64, 1), (16, 33, 64, 2),
          (33, 33, 128, 2), (15, 100, 128, 3), (1, 17, 128, 5), (17, 100, 256, 3), (33, 17, 256, 5), (15, 31, 256, 1),
          (16, 100, 512, 5), (17, 16, 512, 2), (33, 15, 512, 1)]


@pytest.mark.parametrize('R,N,E,ranges', SHAPES)
def test_kernels_vs_fp64(R, N, E, ranges):
    """Forward (lse, target score, loss, trained-row count) and both backward launches, loss scale 0.37 as a host and as a device scalar, d_table
    accumulated onto a non-zero destination whose row 0 keeps its bits, exact zeros in d_prec on untrained rows."""
    ref, _ = check_case(R, N, E, ranges)
    assert ref['count'] > 0


def test_workload_head_size():
    """The flagship head: 64 users x 20 positions against 14 720 items, E = 64, the library's own range count."""
    check_case(1280, 14720, 64, 0)


@pytest.mark.parametrize('R,N,E,ranges', [(17, 33, 64, 1), (33, 100, 128, 5)])
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


@pytest.mark.parametrize('ranges', [1, 3])
def test_large_scores_stay_finite(ranges):
    """prec scaled so that the scores reach about +-100: without max subtraction exp overflows.  Everything finite; lse (and the target score) within
    2e-4 x max |score| -- fp32 rounding of an E <= 512 dot product is about 3e-5 relative at worst."""
    ref, fig = check_case(33, 100, 64, ranges, scale=28.0)
    assert 80 <= np.abs(ref['s']).max() <= 140, np.abs(ref['s']).max()


@pytest.mark.parametrize('ranges', [1, 5])
def test_two_calls_give_the_same_bits(ranges):
    case, _ = reference(33, 100, 64)
    dev = to_dev(case)
    g0 = torch.randn(101, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    outs = []
    for _ in range(2):
        lse, s_tgt, lw = forward(dev, ranges)
        d_prec, d_table = backward(dev, lse, lw, ranges, g0)
        outs.append([t.clone() for t in (lw[:3], lse, s_tgt, d_prec, d_table)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(outs[0][4], g0)


BAD = [dict(E=96), dict(R=0), dict(R=-3), dict(N1=1), dict(ranges=33), dict(ranges=-1)]


@pytest.mark.parametrize('bad', BAD, ids=lambda b: '_'.join(f'{k}{v}' for k, v in b.items()))
def test_invalid_arguments_are_refused_before_any_launch(bad):
    """Unsupported width, R <= 0, N1 < 2, ranges outside 0 .. 32: the library's invalid-argument status from every entry point that takes the
    argument, and every output keeps its fill."""
    from adapter4rec_amd import _lib as L
    E, N1, R, ranges = bad.get('E', 64), bad.get('N1', 40), bad.get('R', 16), bad.get('ranges', 1)
    prec, table = torch.zeros(16, E, device=DEV), torch.zeros(N1, E, device=DEV)
    tgt, m = torch.ones(16, dtype=torch.int32, device=DEV), torch.ones(16, device=DEV)
    outs = [torch.full(s, 7.0, device=DEV) for s in ((16,), (16,), (4,), (16, E), (N1, E))]
    lse, s_tgt, lw, d_prec, d_table = outs
    status = r'status -1 \(invalid argument\)'
    with pytest.raises(RuntimeError, match=status):
        L.score_ce_fwd(prec, table, tgt, m, lse, s_tgt, lw, R, ranges=ranges)
    with pytest.raises(RuntimeError, match=status):
        L.score_ce_bwd(prec, table, tgt, m, lse, lw, 1.0, d_prec, None, R, ranges=ranges)
    if 'ranges' not in bad:                              # (the item launch has no ranges: a wave owns whole item tiles)
        with pytest.raises(RuntimeError, match=status):
            L.score_ce_bwd(prec, table, tgt, m, lse, lw, 1.0, None, d_table, R)
    torch.cuda.synchronize()
    for t in outs:
        assert float((t - 7.0).abs().max()) == 0.0
