"""CPU: the device-side ID batch sampler (--item_tower id --device_sampler 1) -- the properties of the draw rule of a4r_id_sample on its
restatement (tests/id_sample_ref.py: never the user's own item, always 1..item_num, exactly uniform over the rest, independent of the batch),
DeviceIdSampler against BuildTrainDataset in everything deterministic, the flag and the constructor's checks, and the image entry point end to
end on the simulated library with the restatement standing in for _lib.id_sample: two epochs, a resume that repeats the second, the logged
HR@10 against the CPU oracle on the checkpoint.  tests/test_id_sample_gpu.py pins the kernel to the restatement bit for bit."""
import math
import os
import random

import numpy as np
import pytest
import torch

import id_sample_ref as REF
import sim_lib
from test_id_tower_cpu import ID_FLAGS, oracle_hr_id, simulated  # noqa: F401  (simulated: the fixture)


def table(seqs, L):
    t = np.zeros((len(seqs), L), dtype=np.int32)
    for r, s in enumerate(seqs):
        t[r, L - len(s):] = s
    return t


# ------------------------------------------------------------------ the rule
def test_negatives_avoid_the_sequence_and_stay_in_the_catalogue():
    rng = np.random.default_rng(0)
    item_num, L = 40, 21
    seqs = [list(rng.choice(np.arange(1, item_num + 1), n, replace=False)) for n in (21, 2, 5, 12)] + [[40, 1, 40, 1, 7]]
    tab = table(seqs, L)
    for draw in (0, 1, 2 ** 24 - 1):
        ids, mask, err = REF.id_sample(tab, np.arange(len(seqs)), item_num, 99, draw, True)
        assert err == 0 and ids.dtype == np.int64 and mask.dtype == np.float32
        for u, s in enumerate(seqs):
            pad = L - len(s)
            np.testing.assert_array_equal(ids[u, :, 0], [0] * pad + [int(x) for x in s])
            np.testing.assert_array_equal(mask[u], [0] * pad + [1] * (len(s) - 1))
            neg = ids[u, :, 1]
            assert (neg[:pad] == 0).all() and neg[-1] == 0                       # the pad slots and the last slot stay 0
            real = neg[pad:L - 1]
            assert (real >= 1).all() and (real <= item_num).all() and not set(real.tolist()) & set(int(x) for x in s)
    ce, _, err = REF.id_sample(tab, np.arange(len(seqs)), item_num, 99, 0, False)
    assert err == 0 and (ce[:, :, 1] == 0).all() and (ce[:, :, 0] == ids[:, :, 0]).all()


def test_one_candidate_is_always_drawn():
    """m = 1: the sequence {1, 2, 4, 5} in a 5-item catalogue leaves item 3."""
    tab = table([[1, 2, 4, 5], [5, 4, 2, 1, 1, 2]], 8)
    for draw in range(50):
        ids, _, err = REF.id_sample(tab, [0, 1], 5, 7, draw, True)
        assert err == 0
        assert ids[0, 4:7, 1].tolist() == [3, 3, 3] and ids[1, 2:7, 1].tolist() == [3] * 5 and ids[:, 7, 1].tolist() == [0, 0]


def test_a_row_does_not_depend_on_the_rest_of_the_batch():
    rng = np.random.default_rng(1)
    item_num, L = 300, 21
    seqs = [list(rng.choice(np.arange(1, item_num + 1), int(rng.integers(2, 22)), replace=False)) for _ in range(9)]
    tab = table(seqs, L)
    alone = [REF.id_sample(tab, [u], item_num, 5, 3, True) for u in range(9)]
    rows = [8, 3, 3, 0, 7, 1, 2, 6, 5, 4, 3]
    ids, mask, err = REF.id_sample(tab, rows, item_num, 5, 3, True)
    assert err == 0
    for b, u in enumerate(rows):
        np.testing.assert_array_equal(ids[b], alone[u][0][0])
        np.testing.assert_array_equal(mask[b], alone[u][1][0])
    other = REF.id_sample(tab, rows, item_num, 5, 4, True)[0]
    assert (other[:, :, 0] == ids[:, :, 0]).all() and (other[:, :, 1] != ids[:, :, 1]).any()


def test_errors_are_counted_and_leave_the_neighbours_alone():
    tab = table([[1, 2, 3], [2, 3], [1, 2, 3, 3]], 4)                             # item_num 3: users 0 and 2 have no candidate
    ids, mask, err = REF.id_sample(tab, [1, 0, 5, 1, -1, 2], 3, 1, 0, True)
    assert err == 4
    assert ids[1, :, 0].tolist() == [0, 1, 2, 3] and (ids[1, :, 1] == 0).all() and mask[1].tolist() == [0, 1, 1]
    assert (ids[2] == 0).all() and (mask[2] == 0).all() and (ids[4] == 0).all()
    np.testing.assert_array_equal(ids[0], ids[3])
    assert ids[0, :, 0].tolist() == [0, 0, 2, 3] and ids[0, :, 1].tolist() == [0, 0, 1, 0]
    assert REF.id_sample(tab, [1, 0, 5], 3, 1, 0, False)[2] == 1                  # nothing drawn: only the row out of range counts


@pytest.mark.parametrize('name', ['twelve', 'repeats', 'full'])
def test_negatives_are_uniform_over_the_candidates(name):
    """400 draws of every position of one user: chi-square over the m candidates against the uniform law, bound = mean + 4 standard deviations of
    a chi-square with m - 1 degrees of freedom ((m - 1) + 4 sqrt(2 (m - 1))).  Measured: twelve 43.5 (bound 71.4), repeats 27.1 (82.9),
    full 32.1 (57.9)."""
    item_num, L, seed = 50, 21, 12345
    rng = np.random.default_rng(2)
    seq = dict(twelve=[int(x) for x in rng.choice(np.arange(1, 51), 12, replace=False)], repeats=[7, 7, 3, 50, 1],
               full=[int(x) for x in np.random.default_rng(3).choice(np.arange(1, 51), 21, replace=False)])[name]
    tab = table([[1, 2], seq], L)                                                 # (user row 1: the row is part of the hash's counter)
    counts = np.zeros(item_num + 1)
    for draw in range(400):
        neg, m = REF.user_negatives(tab[1], 1, item_num, seed, draw)
        for x in neg[L - len(seq):L - 1]:
            counts[x] += 1
    cand = sorted(set(range(1, item_num + 1)) - set(seq))
    assert m == len(cand) and counts.sum() == 400 * (len(seq) - 1) and counts[sorted(set(seq))].sum() == 0 and counts[0] == 0
    exp = counts.sum() / m
    chi2 = float(((counts[cand] - exp) ** 2 / exp).sum())
    print(f'{name}: m = {m}, chi-square {chi2:.1f}, bound {(m - 1) + 4 * math.sqrt(2 * (m - 1)):.1f}')
    assert chi2 <= (m - 1) + 4 * math.sqrt(2 * (m - 1))


# ------------------------------------------------------------------ the sampler class
@pytest.fixture
def mirrored(monkeypatch):
    from adapter4rec_amd import _lib
    monkeypatch.setattr(_lib, 'id_sample', REF.lib_id_sample)


def test_sampler_equals_build_train_dataset_in_everything_deterministic(mirrored):
    """Positives, pad layout, log_mask, the zero last negative, batch cuts (the last one short), and the negatives outside the user's items."""
    from adapter4rec_amd.data_utils import BuildTrainDataset, DeviceIdSampler
    rng = np.random.default_rng(4)
    item_num, L = 60, 21
    u2seq = {u: [int(x) for x in rng.choice(np.arange(1, item_num + 1), int(rng.integers(2, 22)), replace=False)] for u in range(11)}
    u2seq[3] = [9, 9, 4, 9, 60, 1]
    ds = BuildTrainDataset(u2seq, None, item_num, 20, use_modal=False)
    sm = DeviceIdSampler(u2seq, item_num, 20, 'cpu', seed=5)
    with pytest.raises(RuntimeError, match='set_epoch'):
        next(sm.batches(4))
    order = [int(x) for x in rng.permutation(11)]
    sm.set_epoch(2, order)
    got = list(sm.batches(4))
    assert [int(m.shape[0]) for _, m in got] == [4, 4, 3]
    random.seed(0)
    for k, (flat, mask) in enumerate(got):
        assert flat.dtype == torch.int64 and flat.dim() == 1 and mask.dtype == torch.float32 and tuple(mask.shape) == (flat.numel() // (2 * L), L - 1)
        ids = flat.view(-1, L, 2)
        for b, u in enumerate(order[4 * k:4 * k + 4]):
            ref_ids, ref_mask = ds[u]
            np.testing.assert_array_equal(ids[b, :, 0].numpy(), ref_ids[:, 0].numpy())
            np.testing.assert_array_equal(mask[b].numpy(), ref_mask.numpy())
            drawn = ref_ids[:, 1] != 0
            np.testing.assert_array_equal((ids[b, :, 1] != 0).numpy(), drawn.numpy())              # the same slots hold a negative
            assert ids[b, -1, 1] == 0 and not set(ids[b, :, 1][drawn].tolist()) & set(u2seq[u])
    sm.set_epoch(2, order)
    again = list(sm.batches(4))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, again))
    sm.set_epoch(3, order)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(got, sm.batches(4)))
    ce = DeviceIdSampler(u2seq, item_num, 20, 'cpu', seed=5, negatives=False)
    ce.set_epoch(2, order)
    for (flat, mask), (f2, m2) in zip(got, ce.batches(4)):
        assert torch.equal(f2.view(-1, 2)[:, 0], flat.view(-1, 2)[:, 0]) and not f2.view(-1, 2)[:, 1].any() and torch.equal(mask, m2)


def test_sampler_constructor_checks():
    from adapter4rec_amd.data_utils import DeviceIdSampler
    with pytest.raises(ValueError, match='no negative'):
        DeviceIdSampler({0: [1, 2], 1: [1, 2, 3, 4, 5, 5]}, 5, 20, 'cpu')                           # user 1: m = 0
    DeviceIdSampler({0: [1, 2], 1: [1, 2, 3, 4, 5, 5]}, 5, 20, 'cpu', negatives=False)               # (nothing is drawn: no candidate is needed)
    with pytest.raises(ValueError, match='22 items'):
        DeviceIdSampler({0: list(range(1, 23))}, 100, 20, 'cpu')                                   # longer than L = 21
    with pytest.raises(ValueError, match='outside 1'):
        DeviceIdSampler({0: [1, 101]}, 100, 20, 'cpu')
    with pytest.raises(ValueError, match='max_seq_len'):
        DeviceIdSampler({0: [1, 2]}, 100, 256, 'cpu')
    sm = DeviceIdSampler({0: [1, 2]}, 100, 20, 'cpu')
    with pytest.raises(ValueError, match='epoch'):
        sm.set_epoch(2 ** 24, [0])


def test_sampler_reports_the_error_word(monkeypatch):
    """A stand-in that reports a bad row: the word posted by one batch raises at the next look, as the engine's does."""
    from adapter4rec_amd import _lib
    from adapter4rec_amd.data_utils import DeviceIdSampler

    def bad(seqs, rows, item_num, seed, draw, negatives, ids, log_mask, err):
        ids.zero_(), log_mask.zero_()
        err[0] = 2
    monkeypatch.setattr(_lib, 'id_sample', bad)
    sm = DeviceIdSampler({0: [1, 2], 1: [3, 4]}, 100, 20, 'cpu')
    sm.set_epoch(1, [0, 1])
    it = sm.batches(1)
    next(it)
    with pytest.raises(IndexError, match='2 rows'):
        next(it)


def test_binding_checks_its_arguments_before_the_call():
    from adapter4rec_amd import _lib
    seqs, rows = torch.zeros(3, 21, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    ids, mask, err = torch.zeros(4, 21, 2, dtype=torch.int64), torch.zeros(4, 20), torch.zeros(1, dtype=torch.int32)
    for bad, match in ((dict(seqs=seqs.long()), 'seqs'), (dict(rows=rows.long()), 'rows'), (dict(ids=ids.int()), 'ids'), (dict(ids=ids[:3]), 'ids'),
                       (dict(log_mask=mask.double()), 'log_mask'), (dict(log_mask=mask[:, :19]), 'log_mask'), (dict(draw=2 ** 24), 'draw'),
                       (dict(item_num=0), 'item_num'), (dict(seqs=torch.zeros(3, 257, dtype=torch.int32)), 'L = 257'),
                       (dict(err=torch.zeros(2, dtype=torch.int32)), 'err')):
        kw = dict(seqs=seqs, rows=rows, item_num=50, seed=1, draw=0, negatives=True, ids=ids, log_mask=mask, err=err)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            _lib.id_sample(**kw)
    with pytest.raises(RuntimeError, match='device tensors'):                                      # no CPU fallback
        _lib.id_sample(seqs, rows, 50, 1, 0, True, ids, mask, err)


# ------------------------------------------------------------------ the flag and the runner
def test_parser_takes_the_flag():
    from adapter4rec_amd.cv.parameters import parse_args
    assert parse_args([]).device_sampler == 0
    assert parse_args(['--item_tower', 'id', '--device_sampler', '1']).device_sampler == 1


def test_flag_with_a_modal_tower_raises():
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.parameters import parse_args
    args = parse_args(['--item_tower', 'modal', '--device_sampler', '1'])
    with pytest.raises(NotImplementedError, match='--device_sampler 1'):
        RA.train(args, True, 0, None, None, '.', 0.0)


def sampler_two_epochs_resume_and_oracle_hr(tmp_path, monkeypatch, dtype='fp32', loss='bce'):
    """--item_tower id --device_sampler 1 through the image entry point: two epochs in batches of [16, 16, 8] with no DataLoader built, the
    logged validation HR@10 against the oracle on the saved checkpoint, then a resume from epoch 1 that repeats the uninterrupted run's second
    epoch (the draw is keyed by the epoch: no sampler state in the checkpoint).  -> the negatives columns the engine received."""
    import test_cv_run as CR
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.engine_id import IdRecEngine
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + ID_FLAGS + ['--device_sampler', '1', '--loss', loss]
    common[common.index('--compute_dtype') + 1] = dtype

    def no_loader(*a, **k):
        raise AssertionError('--device_sampler 1 built a DataLoader')
    monkeypatch.setattr(RA, 'DataLoader', no_loader)
    seen, real_fwd = [], IdRecEngine.train_forward

    def fwd(self, sample_items, log_mask):
        seen.append(sample_items.detach().reshape(-1, 2).cpu().clone())
        return real_fwd(self, sample_items, log_mask)
    monkeypatch.setattr(IdRecEngine, 'train_forward', fwd)
    a = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--epoch', '2'], monkeypatch, a)
    assert a['batch'] == [16, 16, 8] * 2, a['batch']
    assert all(np.isfinite(a['loss']))
    ckpts = sorted(os.path.join(dp, f) for dp, _, fs in os.walk('.') for f in fs if f.endswith('.pt'))
    names = [os.path.basename(c) for c in ckpts]
    assert names[0] == 'epoch-1.pt', ckpts
    sd = torch.load(ckpts[-1], map_location='cpu', weights_only=False)['model_state_dict']
    hr = oracle_hr_id(sd, data)
    valids = [h for m, h in a['eval'] if m == 'valid']
    assert abs(valids[len(names) - 1] - hr) < 1e-3, (valids, hr)
    if len(ckpts) > 1:
        os.remove(ckpts[1])
    first = list(seen)
    del seen[:]
    b = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--epoch', '1', '--load_ckpt_name', 'epoch-1.pt'], monkeypatch, b)
    assert b['batch'] == [16, 16, 8]
    np.testing.assert_allclose(b['loss'], a['loss'][3:], rtol=2e-3, atol=2e-3)
    assert len(first) == 6 and len(seen) == 3 and all(torch.equal(x, y) for x, y in zip(first[3:], seen))      # the very batches of epoch 2
    return first


def test_runner_simulated_two_epochs_resume_oracle_hr(simulated, mirrored, tmp_path, monkeypatch):  # noqa: F811
    import test_cv_run as CR
    import adapter4rec_amd.engine_id as EI
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    batches = sampler_two_epochs_resume_and_oracle_hr(tmp_path, monkeypatch)
    assert all((b[:, 1] != 0).any() for b in batches)
