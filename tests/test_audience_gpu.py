"""a4r_topk_users on the MI355X (include/a4r_audience.h): exact lists against the fp64 restatement (tests/audience_ref.py, run on the device), bit
equality with a4r_topk_items both ways round, the seen-list rules, random tables against fp64, determinism across grids; user_vectors / audience
/ write_audience on the ID model, --mode audience through the image entry point, and the tie between --mode recommend and --mode audience."""
import glob
import logging
import os

import numpy as np
import pytest
import torch

import audience_ref as AR
from topk_ref import csr as csr32

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BITS = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return a.to(DEV) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_users(item, users, query, k, ptr, flat, elig=None):
    """item / users: device tensors; query, ptr, flat, elig: numpy -> (rows, scores) numpy"""
    from adapter4rec_amd import _lib as L
    q = dev(np.asarray(query, dtype=np.int64).astype(np.int32))
    rows = torch.empty(q.numel(), k, dtype=torch.int32, device=DEV)
    sc = torch.empty(q.numel(), k, dtype=torch.float32, device=DEV)
    L.topk_users(item, q, users, dev(np.asarray(ptr, np.int64)), dev(np.asarray(flat, np.int32)), None if elig is None else dev(np.asarray(elig, np.uint8)), k, rows, sc)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), sc.cpu().numpy()


def assert_exact(got, want):
    """rows equal, scores equal bit for bit (the restatement's fp64 scores are exact fp32 numbers on integer tables)"""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(BITS(got[1]), BITS(want[1]))


# (K, E, U1, Q).  U1: one row; one tile + 1; one full round of the four waves + 1; several ranges (1025: 16 steps in all, 14720: 32 ranges and the
# merge at Q <= 40).  Q: one row of a workgroup, a full one, one more, three workgroups with a partial last.  K = 256: 64 free slots, the
# compaction trigger in the first steps; K > U1 - 1: short lists.  Every E.
EXACT_CASES = [(1, 64, 2, 1), (10, 128, 17, 16), (10, 256, 65, 17), (256, 512, 65, 40), (100, 64, 1025, 40), (256, 128, 1025, 17), (100, 512, 14720, 16),
               (10, 64, 14720, 40), (256, 256, 14720, 1), (1, 128, 2, 17)]


@pytest.mark.parametrize('K,E,U1,Q', EXACT_CASES)
def test_users_exact_on_integer_tables(K, E, U1, Q):
    rng = np.random.default_rng(K * 7 + E + U1 + Q)
    N1 = 50
    item_np = AR.integer_table(rng, N1, E)
    item_np[7] = 0                                                                 # an all-zero query: every score 0, the smallest rows
    query = rng.integers(1, N1, size=Q)
    query[::6] = 7
    item, users = dev(item_np), dev(AR.integer_table(rng, U1, E))
    ptr, flat = AR.csr_of_mask(rng.random((U1, N1)) < 0.1)
    elig = rng.random(U1) < 0.6
    for e in (None, elig):
        assert_exact(run_users(item, users, query, K, ptr, flat, e), AR.audience_reference(item, users, query, K, ptr, flat, e))


def test_users_exact_with_every_column_appended_at_every_step():
    """User rows whose first entry is the row's tile: item 1 = e0 scores every row its tile (ascending with the tile: all 64 lane columns of every
    step beat the threshold, 64 appends per query and step but for the seen rows, a compaction at every step at K = 64), item 3 = -e0 descends
    (nothing is appended after the first step), item 2 = 0 ties everywhere (the order falls to the rows); query ids 0 and N1 are dead.  4099
    queries: 8 ranges of 4 steps each, the merge, a partial last workgroup."""
    K, E, U1, N1, Q = 64, 64, 2049, 20, 4099
    users = np.zeros((U1, E), np.float32)
    users[1:, 0] = (np.arange(1, U1) - 1) // 16
    item = np.zeros((N1, E), np.float32)
    item[1, 0], item[3, 0] = 1, -1
    lists = [[1, 3] if r % 7 == 0 else ([2] if r % 5 == 0 else []) for r in range(U1)]
    ptr, flat = AR.csr(lists)
    kinds = np.array([1, 2, 3, 0, N1])
    item, users = dev(item), dev(users)
    ri, rs = AR.audience_reference(item, users, kinds, K, ptr, flat)                # once per distinct query
    r = np.arange(Q) % kinds.size
    got = run_users(item, users, kinds[r], K, ptr, flat)
    assert_exact(got, (ri[r], rs[r]))
    assert ri[0, 0] == U1 - 16 and ri[1, 0] == 1 and ri[2, 0] == 1 and (ri[3:] == 0).all()      # the top tile's first row; ties: the first row


@pytest.mark.parametrize('E', (64, 256))
def test_users_equal_the_role_swapped_topk_items_bit_for_bit(E):
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(E)
    N1, U1, Q, K = 300, 4097, 33, 10
    item = dev(rng.standard_normal((N1, E)).astype(np.float32))
    users = dev(rng.standard_normal((U1, E)).astype(np.float32))
    query = rng.integers(1, N1, size=Q)
    got = run_users(item, users, query, K, np.zeros(U1 + 1, np.int64), np.zeros(0, np.int32))
    ids = torch.empty(Q, K, dtype=torch.int32, device=DEV)
    sc = torch.empty(Q, K, dtype=torch.float32, device=DEV)
    L.topk_items(item[dev(query)].contiguous(), users, torch.zeros(Q + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), K, ids, sc)
    torch.cuda.synchronize()
    assert_exact(got, (ids.cpu().numpy(), sc.cpu().numpy()))
    assert (got[0] != 0).all()


def test_users_and_items_list_the_same_triples():
    """40 users, 60 items, seen lists of 0 .. 12 items: a4r_topk_users over all items and a4r_topk_items over all users, K = 64 (every pair that
    may be listed is), the same lists as the users' exclusion -- the same set of (user, item, score bits)."""
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(40)
    n_users, n_items, E, K = 40, 60, 64, 64
    item = dev(rng.standard_normal((n_items + 1, E)).astype(np.float32))
    users = dev(np.concatenate([np.zeros((1, E), np.float32), rng.standard_normal((n_users, E)).astype(np.float32)]))
    lists = [[]] + [sorted(rng.choice(np.arange(1, n_items + 1), size=int(rng.integers(0, 13)), replace=False).tolist()) for _ in range(n_users)]
    ptr, flat = AR.csr(lists)
    rows, sc = run_users(item, users, np.arange(1, n_items + 1), K, ptr, flat)
    by_item = {(int(r) - 1, i + 1, int(b)) for i in range(n_items) for r, b in zip(rows[i], BITS(sc[i])) if r != 0}
    p32, f32 = csr32(lists[1:])
    ids = torch.empty(n_users, K, dtype=torch.int32, device=DEV)
    s2 = torch.empty(n_users, K, dtype=torch.float32, device=DEV)
    L.topk_items(users[1:].contiguous(), item, dev(p32), dev(f32), K, ids, s2)
    torch.cuda.synchronize()
    ids, s2 = ids.cpu().numpy(), s2.cpu().numpy()
    by_user = {(u, int(i), int(b)) for u in range(n_users) for i, b in zip(ids[u], BITS(s2[u])) if i != 0}
    assert by_item == by_user and len(by_item) == n_users * n_items - sum(len(l) for l in lists)


def test_users_seen_list_rules():
    rng = np.random.default_rng(8)
    N1, U1, E, K = 1200, 200, 64, 12
    item_np, users_np = AR.integer_table(rng, N1, E), AR.integer_table(rng, U1, E)
    qa, qb, qc, qd = 5, 1100, 77, 300
    users_np[1:9] = -item_np[qc]                                                   # the rows with the hand-made lists below: last for query qc
    every = np.array([qa, qb, qc, qd])
    others = lambda n, lo, hi: rng.choice(np.setdiff1d(np.arange(lo, hi), every), size=n, replace=False).tolist()
    lists = [others(int(rng.integers(0, 9)), 1, N1) for _ in range(U1)]
    lists[1] = []                                                                  # (with qd below: length 1, the query alone)
    lists[2] = [qa] + others(262, 6, N1)                                           # length 264, query qa first
    lists[3] = others(498, 1, qb) + [qb] + others(500, qb + 1, 5000)               # length 1 000, query qb in the middle (ids beyond N1 behind it)
    lists[4] = others(998, 1, qb) + [qb]                                           # length 1 000, query qb last
    lists[5] = [qa, qa, qa, 9, 9, qb, qb]                                          # repeats
    lists[6] = [-4, 0, qa, 5000, 2 ** 31 - 1]                                      # ids that are no item around the query
    lists[7] = others(263, 6, N1)                                                  # length 264 without qa or qb: listed
    lists[8] = others(999, 1, N1)                                                  # length 1 000 without qa or qb: listed
    s = item_np[qc].astype(np.float64) @ users_np.astype(np.float64).T
    order = 1 + np.lexsort((np.arange(1, U1), -s[1:]))                             # the rows of query qc, best first, ties by row
    assert order[:4 * K].min() > 8
    for r in order[:3 * K]:                                                        # the popular item: its 3 K best rows have all seen it
        lists[r] = lists[r] + [qc]
    for r in range(1, U1):                                                         # an item every row has seen
        lists[r] = sorted(lists[r] + [qd])
    lists[0] = [qa, qb, qc]                                                        # a list for the pad row: never read, row 0 never listed
    assert [len(lists[r]) for r in (1, 2, 3, 4, 7, 8)] == [1, 264, 1000, 1000, 264, 1000] and lists[2][0] == qa and lists[4][-1] == qb and lists[3][499] == qb
    ptr, flat = AR.csr(lists)
    item, users = dev(item_np), dev(users_np)
    query = np.array([qa, qb, qc, qd, 0, -5, N1, qa, 2 ** 31 - 1])
    dead = [3, 4, 5, 6, 8]                                                         # seen by every row; ids that are no item
    got = run_users(item, users, query, K, ptr, flat)
    assert_exact(got, AR.audience_reference(item, users, query, K, ptr, flat))
    rows, sc = got
    full = run_users(item, users, query, 256, ptr, flat)[0]                        # K = 256 > U1 - 1: everything that may be listed, then pads
    assert not set(full[0]) & {2, 5, 6} and {1, 3, 4, 7, 8} <= set(full[0])       # qa: first in a list, repeated, among ids that are no item
    assert not set(full[1]) & {3, 4, 5} and {1, 2, 6, 7, 8} <= set(full[1])       # qb: middle and last of 1 000, repeated
    assert (full[0] != 0).sum() == U1 - 1 - 3 and (full[1] != 0).sum() == U1 - 1 - 3 and (full[:, U1 - 1:] == 0).all()
    assert rows[2].tolist() == order[3 * K:4 * K].tolist()                         # the popular item: the next K
    assert (rows[dead] == 0).all() and np.isneginf(sc[dead]).all()
    np.testing.assert_array_equal(rows[0], rows[7])                                # a repeated query id: an equal row
    np.testing.assert_array_equal(BITS(sc[0]), BITS(sc[7]))
    # elig: one eligible row; none among a query's unseen rows
    one = np.zeros(U1, np.uint8)
    one[[0, 7]] = 1                                                                # (row 0 is never listed, eligible or not)
    got = run_users(item, users, query, K, ptr, flat, one)
    assert_exact(got, AR.audience_reference(item, users, query, K, ptr, flat, one))
    assert got[0][0].tolist() == [7] + [0] * (K - 1) and got[0][1].tolist() == [7] + [0] * (K - 1)
    assert got[1][0, 0] == np.float32(item_np[qa].astype(np.float64) @ users_np[7].astype(np.float64))
    none = np.zeros(U1, np.uint8)
    none[[2, 5, 6]] = 1                                                            # exactly the rows that have seen qa
    got = run_users(item, users, query, K, ptr, flat, none)
    assert_exact(got, AR.audience_reference(item, users, query, K, ptr, flat, none))
    assert (got[0][0] == 0).all() and np.isneginf(got[1][0]).all() and set(got[0][1]) == {2, 6, 0}
    # an unsorted list can mislist, never stray: the launch completes, lists rows of the table only, and dead queries stay dead
    ptr_u, flat_u = AR.csr([l[::-1] for l in lists])
    r_u = run_users(item, users, query, K, ptr_u, flat_u)[0]
    assert ((r_u >= 0) & (r_u < U1)).all() and (r_u[[4, 5, 6, 8]] == 0).all()


@pytest.mark.parametrize('K,E,U1,Q,seed', AR.RANDOM_CASES)
def test_users_random_tables_against_fp64(K, E, U1, Q, seed):
    """Every returned score within E 2^-24 sum |a b| of the fp64 score; every decided position (the restatement's scores at K + 1 depth separated
    from both neighbours by more than 2 max b) holds the restatement's row; at least 0.90 of the positions are decided (the restatement alone
    gives 1.000 / 0.963 / 0.972 / 0.958 / 0.975 on these cases: tests/test_audience_cpu.py)."""
    item_np, users_np, query, mask = AR.random_case(K, E, U1, Q, seed)
    ptr, flat = AR.csr_of_mask(mask)
    item, users = dev(item_np), dev(users_np)
    rows, sc = run_users(item, users, query, K, ptr, flat)
    s64 = AR.scores64(item, users, query).cpu().numpy()
    b = AR.bounds(item, users, query)
    ri, rs = AR.audience_reference(item, users, query, K + 1, ptr, flat)
    assert (rows != 0).all() and not mask[rows, query[:, None]].any()              # full lists; no row has seen its query
    at = np.arange(Q)[:, None]
    err = np.abs(sc.astype(np.float64) - s64[at, rows])
    print(f'K = {K}, E = {E}: largest |score - fp64| / b = {float((err / b[at, rows]).max()):.3f}')
    assert np.all(err <= b[at, rows])
    sure = AR.decided(rs, b.max(1))
    print(f'decided positions: {sure.mean():.3f}')
    assert sure.mean() >= 0.90
    np.testing.assert_array_equal(rows[sure], ri[:, :K][sure])
    top = np.argsort(-s64[0, 1:], kind='stable')[:3 * K] + 1                       # the popular item: none of its 3 K best rows is listed
    assert not set(top) & set(rows[0])


def test_users_deterministic_and_grid_independent():
    rng = np.random.default_rng(4)
    Q, N1, U1, E, K = 16400, 257, 4097, 64, 10
    item = dev(rng.standard_normal((N1, E)).astype(np.float32))
    users = dev(rng.standard_normal((U1, E)).astype(np.float32))
    ptr, flat = AR.csr_of_mask(rng.random((U1, N1)) < 0.08)
    query = rng.integers(1, N1, size=Q)
    a = run_users(item, users, query, K, ptr, flat)
    assert_exact(run_users(item, users, query, K, ptr, flat), a)
    for r in (0, 12345, Q - 1):                                                   # alone: 1 workgroup x 32 ranges + the merge; in the batch: 1 range
        r1, s1 = run_users(item, users, query[r:r + 1], K, ptr, flat)
        np.testing.assert_array_equal(r1[0], a[0][r])
        np.testing.assert_array_equal(BITS(s1[0]), BITS(a[1][r]))


def test_users_argument_errors_launch_nothing():
    import ctypes as C
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    Q, N1, U1 = 16, 101, 77
    item, users = torch.randn(N1, 128, device=DEV), torch.randn(U1, 128, device=DEV)
    query = torch.arange(1, Q + 1, dtype=torch.int32, device=DEV)
    ptr = torch.zeros(U1 + 1, dtype=torch.int64, device=DEV)
    flat = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows = torch.full((Q, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((Q, 257), 7.0, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    f = lib.a4r_topk_users
    assert (f.restype, f.argtypes) == L.AUDIENCE_SIGNATURES['a4r_topk_users']
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    # (item offset, users offset, ws offset, ptr offset, Q, N1, U1, E, K)
    for io, uo, wo, po, q, n1, u1, E, K in ((0, 0, 0, 0, Q, N1, U1, 128, 0), (0, 0, 0, 0, Q, N1, U1, 128, 257), (0, 0, 0, 0, Q, N1, U1, 96, 10), (4, 0, 0, 0, Q, N1, U1, 64, 10),
                                            (0, 8, 0, 0, Q, N1, U1, 64, 10), (0, 0, 4, 0, Q, N1, U1, 64, 10), (0, 0, 0, 4, Q, N1, U1, 64, 10), (0, 0, 0, 0, 0, N1, U1, 64, 10),
                                            (0, 0, 0, 0, Q, 1, U1, 64, 10), (0, 0, 0, 0, Q, N1, 1, 64, 10)):
        assert f(None, P(item, io), P(query), P(users, uo), P(ptr, po), P(flat), None, P(rows), P(sc), P(ws, wo), q, n1, u1, E, K) == -1, (io, uo, wo, po, q, n1, u1, E, K)
    for null in (1, 2, 3, 4, 5, 7, 8, 9):
        a = [None, P(item), P(query), P(users), P(ptr), P(flat), None, P(rows), P(sc), P(ws), Q, N1, U1, 128, 10]
        a[null] = None
        assert f(*a) == -1, null
    torch.cuda.synchronize()
    assert bool((rows == 7).all()) and bool((sc == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ API level

class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _id_model(U=45):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    model, args, item_num, _, eval_seq, hist = _id_model_and_users(U)
    model = model.to(DEV)
    return model, args, item_num, get_itemId_embeddings(model, item_num, 256, args, 0), eval_seq, hist


def test_audience_on_the_id_model_against_the_restatement(monkeypatch):
    from adapter4rec_amd.data_utils.metrics import audience, audience_seen_csr, recommend, user_vectors
    model, args, item_num, emb, eval_seq, _ = _id_model()
    n, k = len(eval_seq), 7
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '25')                                # several batches of users and of query items
    uv = user_vectors(model, eval_seq, emb, args)
    assert uv.dtype == torch.float32 and tuple(uv.shape) == (n, emb.shape[1]) and uv.device == emb.device
    ids, sc = audience(model, eval_seq, emb, k, args)
    assert ids.dtype == torch.long and tuple(ids.shape) == (item_num, k) == tuple(sc.shape) and ids.device == emb.device
    table = torch.cat([torch.zeros(1, emb.shape[1], device=DEV), uv])
    ptr, flat = audience_seen_csr(eval_seq, n)
    query = np.arange(1, item_num + 1)
    ri, rs = AR.audience_reference(emb, table, query, k + 1, ptr, flat)
    b = AR.bounds(emb, table, query)
    sure = AR.decided(rs, b.max(1))
    ids_np, sc_np = ids.cpu().numpy(), sc.cpu().numpy()
    assert sure.mean() > 0.9
    np.testing.assert_array_equal(ids_np[sure], ri[:, :k][sure] - 1)
    assert np.all((np.abs(sc_np - rs[:, :k]) <= b.max(1)[:, None])[sure])
    for u in range(n):                                                             # a user is never listed for an item of the user's sequence
        assert not (ids_np[np.asarray(eval_seq[u]) - 1] == u).any()
    some = np.array([7, 3, 3, item_num, 0, item_num + 1])
    elig = np.zeros(n, bool)
    elig[[2, 5, 11]] = True
    i2, s2 = audience(model, eval_seq, emb, k, args, item_ids=some, seen={u: [] for u in range(n)}, eligible=elig)
    assert set(i2[0].tolist()) == {2, 5, 11, -1} and (i2[:4, 3:] == -1).all() and torch.isneginf(s2[:4, 3:]).all() and torch.equal(i2[1], i2[2])
    assert (i2[4:] == -1).all() and torch.isneginf(s2[4:]).all()
    # the two modes tied together: user u's recommended item i lists u with the same score bits, or i's list is full of rows that key higher
    K = 5
    rec_i, rec_s = recommend(model, eval_seq, emb, K, args)
    aud_u, aud_s = audience(model, eval_seq, emb, K, args)
    rec_i, rec_s, aud_u, aud_s = rec_i.cpu().numpy(), rec_s.cpu().numpy(), aud_u.cpu().numpy(), aud_s.cpu().numpy()
    found = 0
    for u in range(n):
        for i, s in zip(rec_i[u], rec_s[u]):
            if i == 0:
                continue
            at = np.flatnonzero(aud_u[i - 1] == u)
            if at.size:
                assert BITS(aud_s[i - 1, at[0]]) == BITS(s), (u, i)
                found += 1
            else:
                assert (aud_u[i - 1] >= 0).all() and all(x > s or (x == s and v < u) for x, v in zip(aud_s[i - 1], aud_u[i - 1])), (u, i)
    print(f'{found} recommended (user, item) pairs found in the item\'s audience')
    assert found > 0


def test_write_audience_round_trips(tmp_path):
    from adapter4rec_amd.data_utils.metrics import audience, write_audience
    model, args, item_num, emb, eval_seq, hist = _id_model()
    n, k = len(eval_seq), 5
    hist[4] = torch.LongTensor(np.arange(1, item_num + 1))                         # a user who has seen everything -- beyond any 264-id list
    user_names = [f'U{u}' for u in range(n)]
    item_names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    elig = np.zeros(n, bool)
    elig[[4, 9, 20]] = True
    query = np.array([4, int(eval_seq[9][-1]), 2, item_num])
    hist[20] = torch.LongTensor(np.array([int(eval_seq[9][-1])]))                  # the second query: seen by all three eligible users -> no line
    path, log = str(tmp_path / 'aud.tsv'), _Log()
    assert write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, item_ids=query, eligible=elig, Log_file=log) == path
    seen = {u: np.concatenate([np.asarray(hist[u]), np.asarray(eval_seq[u][-1:])]) for u in range(n)}
    ids, sc = audience(model, eval_seq, emb, k, args, item_ids=query, seen=seen, eligible=elig)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    keep_rows = [r for r in range(4) if ids[r, 0] >= 0]
    assert (ids[1] == -1).all() and 1 not in keep_rows and len(keep_rows) >= 1 and not (ids == 4).any()
    assert [r[0] for r in rows] == [f'N{int(query[r])}' for r in keep_rows]
    for r, row in zip(keep_rows, rows):
        keep = ids[r] >= 0
        assert row[1].split(' ') == [f'U{u}' for u in ids[r][keep]] and set(ids[r][keep]) <= {9, 20}
        assert [np.float32(x) for x in row[2].split(' ')] == sc[r][keep].tolist()      # %.9g round-trips fp32
    assert len(log.lines) == 1 and log.lines[0].endswith('-> ' + path)
    assert log.lines[0].startswith(f'audience   top-5 lists of 4 items over {n} users (3 eligible), {len(keep_rows)} with a user, mean best score ')


def test_cv_id_runner_mode_audience(tmp_path, monkeypatch):
    """The image entry point with --item_tower id on the GPU: one epoch, then --mode audience from its checkpoint writes the default path and the
    log line; every line's users have not seen the line's item, and the scores descend."""
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.data_utils import read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    orig_setup = RA.setuplogger

    def setup(*a, **kw):                                                          # (_run_cv drops the loggers' handlers after every run)
        out = orig_setup(*a, **kw)
        logging.getLogger('Log_file').addHandler(Keep())
        return out
    monkeypatch.setattr(RA, 'setuplogger', setup)
    rec = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--mode', 'audience', '--load_ckpt_name', 'epoch-1.pt', '--topk', '4'], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == []
    out = os.path.join(os.path.dirname(ck[0]), 'audience_epoch-1.pt.tsv')
    _, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    user_names, item_names = read_behavior_names(os.path.join(data, 'toy', 'users_log.tsv'), name2id, 20, 5)
    N, n = len(item_names) - 1, len(user_names)
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert 0 < len(rows) <= N and [r[0] for r in rows] == [x for x in item_names[1:] if x in {r[0] for r in rows}]      # query order
    seen = {}
    for l in open(os.path.join(data, 'toy', 'users_log.tsv')):
        name, seq = l.rstrip('\n').split('\t')[:2]
        seen[name] = set(seq.split(' ')[-23:])                                      # (read_behaviors keeps a user's last max_seq_len + 3 items)
    for r in rows:
        us, ss = r[1].split(' '), [float(x) for x in r[2].split(' ')]
        assert 1 <= len(us) == len(ss) <= 4 and len(set(us)) == len(us) and set(us) <= set(user_names)
        assert ss == sorted(ss, reverse=True) and all(r[0] not in seen[u] for u in us)
    line = [l for l in lines if l.startswith('audience   ')]
    assert len(line) == 1 and line[0].startswith(f'audience   top-4 lists of {N} items over {n} users ({n} eligible), {len(rows)} with a user, mean best score ')
    assert line[0].endswith('/audience_epoch-1.pt.tsv')
