"""CPU: the cross-entropy head of the ID tower (--loss ce) -- the fp64 restatement the GPU tests compare against (tests/score_ce_ref.py) pinned to
torch's cross_entropy, the flag, the refusals, and the library's host-side queries (range count, workspace size)."""
import numpy as np
import pytest
import torch

import score_ce_ref as CE
import test_id_tower_cpu as CPU


def _case(R, N, E, seed):
    rng = np.random.default_rng(seed)
    prec, table = rng.standard_normal((R, E)) * E ** -0.25, rng.standard_normal((N + 1, E)) * E ** -0.25
    tgt = rng.integers(1, N + 1, R)
    mask = np.ones(R)
    tgt[::5] = 0                                                        # rows without a target
    mask[1::4] = 0                                                      # masked rows
    if R > 3:
        tgt[2], tgt[3] = N, N                                           # the last item, twice
    return prec, table, tgt, mask


@pytest.mark.parametrize('R,N,E', [(1, 1, 8), (7, 3, 16), (33, 100, 64), (40, 17, 32)])
def test_restatement_equals_torch_cross_entropy(R, N, E):
    prec, table, tgt, mask = _case(R, N, E, seed=R + N)
    if R == 1:
        tgt[:], mask[:] = 1, 1
    ref = CE.reference(prec, table, tgt, mask)
    p = torch.from_numpy(prec).requires_grad_(True)
    t = torch.from_numpy(table).requires_grad_(True)
    sel = torch.from_numpy((mask != 0) & (tgt != 0))
    assert int(sel.sum()) == ref['count'] > 0
    logits = p @ t[1:].T
    loss = torch.nn.functional.cross_entropy(logits[sel], torch.from_numpy(tgt)[sel] - 1, reduction='mean')
    dp, dt = torch.autograd.grad(loss, [p, t])
    assert abs(ref['loss'] - float(loss.detach())) <= 1e-12
    np.testing.assert_allclose(ref['lse'], torch.logsumexp(logits, 1).detach().numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(ref['d_prec'], dp.numpy(), atol=1e-12, rtol=0)
    np.testing.assert_allclose(ref['d_table'], dt.numpy(), atol=1e-12, rtol=0)
    assert np.all(ref['d_table'][0] == 0) and np.all(ref['d_prec'][~sel.numpy()] == 0)
    has = tgt != 0
    np.testing.assert_allclose(ref['s_tgt'][has], logits.detach().numpy()[np.flatnonzero(has), tgt[has] - 1], atol=1e-12, rtol=0)


def test_restatement_with_no_trained_row_is_all_zero():
    prec, table, tgt, mask = _case(9, 20, 16, seed=3)
    ref = CE.reference(prec, table, tgt, np.zeros_like(mask))
    assert ref['count'] == 0 and ref['loss'] == 0.0 and not ref['d_prec'].any() and not ref['d_table'].any()
    assert np.isfinite(ref['lse']).all()


def test_parser_accepts_loss_ce_and_defaults_to_bce():
    from adapter4rec_amd.cv.parameters import parse_args
    assert parse_args([]).loss == 'bce'
    assert parse_args(['--loss', 'ce']).loss == 'ce'
    assert parse_args(['--loss', 'bce', '--item_tower', 'id']).loss == 'bce'
    with pytest.raises(SystemExit):
        parse_args(['--loss', 'softmax'])


def test_model_keeps_the_flag_and_the_state_dict():
    from adapter4rec_amd.cv import Model
    a, b = Model(CPU.make_args(loss='ce'), 60, False), Model(CPU.make_args(), 60, False)
    assert a.loss == 'ce' and b.loss == 'bce'
    assert CPU.shapes_of(a) == CPU.shapes_of(b)


def test_ce_with_cpc_raises():
    from adapter4rec_amd.cv import ModelCPC
    with pytest.raises(NotImplementedError, match='--loss ce'):
        ModelCPC(CPU.make_args(arch='cpc', loss='ce'), 60, False)


def test_ce_with_cpc_engine_raises(simulated_engine):
    """The engine refuses on its own as well (it can be built without the model classes' check: arch is its argument)."""
    from adapter4rec_amd.cv import Model
    from adapter4rec_amd.engine_id import IdRecEngine
    model = Model(CPU.make_args(), 60, False)
    with pytest.raises(NotImplementedError, match='--loss ce'):
        IdRecEngine(model, CPU.make_args(loss='ce'), arch='cpc', dtype='fp32')


def test_ce_with_a_modal_tower_raises():
    from adapter4rec_amd.cv import Model

    class Net(torch.nn.Module):
        config = dict(hidden_size=768)

    with pytest.raises(NotImplementedError, match='--loss ce'):
        Model(CPU.make_args(loss='ce'), 60, True, Net())
    Model(CPU.make_args(loss='bce'), 60, True, Net())                   # (the same construction is accepted without the flag)


def test_ce_with_an_unsupported_width_raises(simulated_engine):
    from adapter4rec_amd.cv import Model
    model = Model(CPU.make_args(loss='ce', embedding_dim=32), 60, False)
    with pytest.raises(NotImplementedError, match='--loss ce'):
        model._engine()


@pytest.fixture
def simulated_engine(monkeypatch):
    import adapter4rec_amd.engine as E
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)


@pytest.mark.parametrize('R,N1', [(1, 2), (16, 17), (17, 18), (1280, 14721), (1280, 500001), (100000, 40), (5, 1000001), (40000, 500001)])
def test_range_count_is_bounded(R, N1):
    from adapter4rec_amd import _lib as L
    k = L.score_ce_ranges(R, N1)
    tiles = (N1 - 1 + 15) // 16
    assert 1 <= k <= 32 and k <= tiles
    assert L.SCORE_CE_MAX_RANGES == 32


def test_range_count_refuses_empty_shapes():
    from adapter4rec_amd import _lib as L
    for R, N1 in ((0, 10), (4, 1), (-1, 5)):
        with pytest.raises(ValueError):
            L.score_ce_ranges(R, N1)


@pytest.mark.parametrize('E', [64, 128, 256, 512])
@pytest.mark.parametrize('ranges', [1, 7, 32])
def test_workspace_does_not_grow_with_the_table(E, ranges):
    """No logits matrix: at a fixed range count the scratch is the same for 1 000 and 1 000 000 table rows, and far below R x N1 floats."""
    from adapter4rec_amd import _lib as L
    R = 1280
    small, large = L.score_ce_ws_bytes(R, 1000, E, ranges), L.score_ce_ws_bytes(R, 1000000, E, ranges)
    assert small == large > 0
    assert large <= ranges * R * E * 4
    assert L.score_ce_ws_bytes(R, 1000000, E, 0) <= 32 * R * E * 4 < R * 1000000 * 4


def test_workspace_is_zero_for_refused_arguments():
    from adapter4rec_amd import _lib as L
    for R, N1, E, ranges in ((0, 100, 64, 1), (16, 1, 64, 1), (16, 100, 96, 1), (16, 100, 64, 33), (16, 100, 64, -1)):
        assert L.score_ce_ws_bytes(R, N1, E, ranges) == 0
