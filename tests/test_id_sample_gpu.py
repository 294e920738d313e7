"""GPU: a4r_id_sample against its restatement (tests/id_sample_ref.py), bit for bit -- ids, log_mask and the error word at the shape edges: L = 2
(one position, no negative but the last slot's zero), 21 (the default), 33, 64 / 65 (one lane stride and one element past it), 256 (the
longest row: four elements per lane in the rank-counting sort); B = 1 and 65; users without a pad and of length 2, repeated ids, ids 1 and
item_num, one candidate left (m = 1), repeated and descending rows, a catalogue of 2^31 - 2 items (the high half of the 64 x 64-bit product
carries the draw), draw 0 and 2^24 - 1, negatives off.  The outputs sit between guard rows that must come back untouched."""
import numpy as np
import pytest
import torch

import id_sample_ref as REF

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 2
GUARD_I, GUARD_F, GUARD_E = -7, -3.0, -9


def users(L, item_num, rng):
    """The user kinds above as one int32 [6, L] table of a catalogue of item_num >= L + 1 items."""
    pool = np.arange(1, item_num + 1) if item_num < 10 ** 6 else None

    def distinct(n):
        if pool is not None:
            return [int(x) for x in rng.choice(pool, n, replace=False)]
        out = set()
        while len(out) < n:
            out.add(int(rng.integers(1, item_num + 1)))
        return list(out)
    full = distinct(L)                                                            # no pad (small catalogue of L + 1 items: m = 1)
    rng.shuffle(full)
    two = [item_num, 1]                                                           # length 2: the catalogue's first and last id
    n_rep = max(2, min(L, 9))
    rep = ([1, item_num, 1] + distinct(3) * 3)[:n_rep]                            # repeated ids, ids 1 and item_num
    half = distinct(max(2, L // 2))
    edge = [item_num] * max(2, L - 1)                                             # one id, L - 1 times: d = 1
    desc = sorted(distinct(max(2, L - 3)), reverse=True)
    tab = np.zeros((6, L), dtype=np.int32)
    for r, s in enumerate((full, two, rep, half, edge, desc)):
        s = s[:L]
        tab[r, L - len(s):] = s
    return tab


def run(tab, rows, item_num, seed, draw, negatives):
    """One call between guard rows -> (ids, log_mask, err) as numpy."""
    from adapter4rec_amd import _lib
    B, L = len(rows), tab.shape[1]
    seqs = torch.from_numpy(tab).cuda()
    rws = torch.tensor(rows, dtype=torch.int32, device='cuda')
    ids = torch.full((B + 2, L, 2), GUARD_I, dtype=torch.int64, device='cuda')
    mask = torch.full((B + 2, L - 1), GUARD_F, dtype=torch.float32, device='cuda')
    err = torch.full((3,), GUARD_E, dtype=torch.int32, device='cuda')
    _lib.id_sample(seqs, rws, item_num, seed, draw, negatives, ids[1:B + 1], mask[1:B + 1], err[1:2])
    torch.cuda.synchronize()
    ids, mask, err = ids.cpu().numpy(), mask.cpu().numpy(), err.cpu().numpy()
    assert (ids[0] == GUARD_I).all() and (ids[B + 1] == GUARD_I).all(), 'ids written outside [B, L, 2]'
    assert (mask[0] == GUARD_F).all() and (mask[B + 1] == GUARD_F).all(), 'log_mask written outside [B, L - 1]'
    assert err[0] == GUARD_E and err[2] == GUARD_E
    return ids[1:B + 1], mask[1:B + 1], int(err[1])


def check(tab, rows, item_num, seed, draw, negatives):
    got = run(tab, rows, item_num, seed, draw, negatives)
    want = REF.id_sample(tab, rows, item_num, seed, draw, negatives)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[1].dtype == np.float32 and got[2] == want[2]
    return got


@pytest.mark.parametrize('item_num', ['small', 'big'])
@pytest.mark.parametrize('B', [1, 65])
@pytest.mark.parametrize('L', [2, 21, 33, 64, 65, 256])
def test_kernel_equals_the_restatement(L, B, item_num):
    item_num = L + 1 if item_num == 'small' else BIG                              # small: the user without a pad keeps one candidate
    rng = np.random.default_rng(L * 1000 + B)
    tab = users(L, item_num, rng)
    if B == 1:
        row_sets = [[0], [2]]
    else:
        row_sets = [[5 - (b // 2) % 6 for b in range(B)]]                         # descending, every row twice in a row, the table cycled
    seed = 0x1234_5678_9ABC_DEF0 + L
    for rows in row_sets:
        a = check(tab, rows, item_num, seed, 0, True)
        assert a[2] == 0
        b = check(tab, rows, item_num, seed, 2 ** 24 - 1, True)
        again = run(tab, rows, item_num, seed, 0, True)
        assert all(np.array_equal(x, y) for x, y in zip(a[:2], again[:2])) and again[2] == 0           # two calls, the same bits
        if L > 2 and item_num == BIG:                                             # (small catalogue: the full user has one candidate whatever the draw)
            assert (a[0][:, :, 1] != b[0][:, :, 1]).any()                         # another draw, other negatives
        np.testing.assert_array_equal(a[0][:, :, 0], b[0][:, :, 0])
        c = check(tab, rows, item_num, seed, 5, False)
        assert (c[0][:, :, 1] == 0).all() and c[2] == 0
        drawn = a[0][:, :, 1][a[0][:, :, 1] != 0]
        assert ((drawn >= 1) & (drawn <= item_num)).all()
    if item_num == L + 1 and L > 2:                                                # m = 1: the one item the full user lacks, at every position
        ids = check(tab, [0], item_num, seed, 3, True)[0]
        left = (set(range(1, item_num + 1)) - set(tab[0].tolist())).pop()
        assert ids[0, :-1, 1].tolist() == [left] * (L - 1) and ids[0, -1, 1] == 0


def test_one_user_table():
    tab = np.zeros((1, 21), dtype=np.int32)
    tab[0, 14:] = [3, 9, 3, 1, 50, 7, 7]
    for B in (1, 65):
        ids = check(tab, [0] * B, 50, 11, 2, True)[0]
        assert (ids == ids[0]).all()


def test_high_product_reaches_the_whole_catalogue():
    """item_num = 2^31 - 2: a draw that used the low bits of the product, or a 32-bit product, would not spread over the id range."""
    tab = users(256, BIG, np.random.default_rng(9))
    neg = check(tab, [0, 3, 5], BIG, 77, 1, True)[0][:, :, 1]
    neg = neg[neg != 0]
    assert neg.min() < BIG // 8 and neg.max() > BIG - BIG // 8 and len(np.unique(neg >> 27)) == 16


def test_errors_are_counted_and_the_neighbours_unaffected():
    L = 21
    tab = np.zeros((3, L), dtype=np.int32)
    tab[0, L - 5:] = [1, 2, 3, 4, 5]                                              # item_num 5: no candidate (m = 0)
    tab[1, L - 4:] = [1, 2, 4, 5]                                                 # m = 1: always 3
    tab[2, L - 6:] = [5, 5, 4, 3, 2, 1]                                           # m = 0 with a repeat
    rows = [1, 0, 7, 1, -1, 2, 1, 3]
    ids, mask, err = check(tab, rows, 5, 1, 4, True)
    assert err == 5
    for b in (0, 3, 6):                                                           # the rows next to the bad ones
        assert ids[b, L - 4:, 0].tolist() == [1, 2, 4, 5] and ids[b, L - 4:, 1].tolist() == [3, 3, 3, 0] and mask[b, L - 4:].tolist() == [1, 1, 1]
    assert (ids[[2, 4, 7]] == 0).all() and (mask[[2, 4, 7]] == 0).all()          # out of range: rows of pads
    assert ids[1, L - 5:, 0].tolist() == [1, 2, 3, 4, 5] and (ids[[1, 5], :, 1] == 0).all() and mask[1, L - 5:].tolist() == [1, 1, 1, 1]
    assert check(tab, rows, 5, 1, 4, False)[2] == 3                               # nothing drawn: only the rows out of range count
    assert check(tab, [1, 1], 5, 1, 4, True)[2] == 0                              # the word is overwritten, not accumulated


def test_entry_refuses_bad_arguments_before_launching():
    """The library's own checks (the binding's are tested on the CPU): status -1, outputs untouched."""
    from adapter4rec_amd import _lib
    lib = _lib.lib()
    seqs, rows = torch.zeros(2, 21, dtype=torch.int32, device='cuda'), torch.zeros(4, dtype=torch.int32, device='cuda')
    ids = torch.full((4, 21, 2), GUARD_I, dtype=torch.int64, device='cuda')
    mask, err = torch.full((4, 20), GUARD_F, device='cuda'), torch.full((1,), GUARD_E, dtype=torch.int32, device='cuda')
    ok = dict(seqs=seqs.data_ptr(), n_users=2, L=21, rows=rows.data_ptr(), B=4, item_num=50, draw=0, ids=ids.data_ptr(), mask=mask.data_ptr(),
              err=err.data_ptr())
    for bad in (dict(seqs=0), dict(rows=0), dict(ids=0), dict(mask=0), dict(err=0), dict(L=1), dict(L=257), dict(B=0), dict(n_users=0),
                dict(item_num=0), dict(draw=2 ** 24)):
        a = dict(ok, **bad)
        vals = (0, a['seqs'], a['n_users'], a['L'], a['rows'], a['B'], a['item_num'], 1, a['draw'], 1, a['ids'], a['mask'], a['err'])
        rc = lib.a4r_id_sample(*(t(v) for t, v in zip(_lib.SIGNATURES['a4r_id_sample'][1], vals, strict=True)))
        assert rc == -1, bad
    torch.cuda.synchronize()
    assert (ids == GUARD_I).all() and (mask == GUARD_F).all() and int(err[0]) == GUARD_E
