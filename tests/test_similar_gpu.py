"""a4r_row_inv_norms / a4r_topk_similar on the MI355X (include/a4r_similar.h): exact lists against the fp64 restatement (tests/similar_ref.py, run on
the device) for both metrics, bit equality with a4r_topk_items, random tables against fp64, symmetry, the listing rules, the inverse norms,
determinism across grids, argument errors; similar_items / write_similar_items on the ID model's table."""
import ctypes as C

import numpy as np
import pytest
import torch

import similar_ref as SR
from topk_ref import TRIGGER_N1, TRIGGER_U, csr, trigger_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BITS = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run_similar(emb, query, k, metric='dot', cand=None, min_sim=None):
    from adapter4rec_amd import _lib as L
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(torch.int32).to(DEV)
    ids = torch.empty(q.numel(), k, dtype=torch.int32, device=DEV)
    sc = torch.empty(q.numel(), k, dtype=torch.float32, device=DEV)
    inv = L.row_inv_norms(emb) if metric == 'cos' else None
    L.topk_similar(emb, inv, q, cand, min_sim, k, ids, sc)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def assert_exact(got, want):
    """ids equal, scores equal bit for bit (the restatement's fp64 scores are exact fp32 numbers on these tables)"""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(BITS(got[1]), BITS(want[1]))


# (K, E, N1, Q): N1 - 2 < K (short lists), one and two tiles, one step of four tiles and one item beyond it, the compaction trigger (K = 256: 64 free
# slots, hit in the first steps), 32 item ranges with the merge (Q <= 17), a single range with the decode (Q = 16400)
DOT_CASES = [(1, 64, 2, 1), (7, 128, 17, 15), (7, 64, 18, 17), (10, 64, 65, 16), (10, 256, 66, 16), (256, 512, 17, 16), (64, 256, 14720, 17),
             (256, 64, 14720, 16), (100, 128, 14720, 4096), (10, 64, 14720, 16400)]


@pytest.mark.parametrize('K,E,N1,Q', DOT_CASES)
def test_similar_exact_dot_on_integer_tables(K, E, N1, Q):
    rng = np.random.default_rng(K * 7 + E + N1 + Q)
    query = rng.integers(1, N1, size=Q)
    emb = SR.integer_table(rng, N1, E, zero_rows=query[::5] if N1 > 2 else ())    # an all-zero query: every score 0, the smallest ids
    emb = torch.from_numpy(emb).to(DEV)
    assert_exact(run_similar(emb, query, K, 'dot'), SR.similar_reference(emb, query, K, 'dot'))


def test_similar_exact_dot_with_every_column_appended_at_every_step():
    """topk_ref.trigger_case's table under the dot metric: a query from the top tile scores every item 255 x its tile (ascending with the tile: 64
    appends per row and step, compaction at every step at K = 64), a query from tile 0 scores every item 0 (the order falls to the ids); query
    ids 0 and N1 are dead rows.  32769 queries: one item range, a partial last workgroup."""
    K, E = 64, 64
    emb = torch.from_numpy(trigger_case(E)[0]).to(DEV)
    kinds = np.concatenate([np.arange(TRIGGER_N1 - 16, TRIGGER_N1), np.arange(1, 17), [0, TRIGGER_N1]])
    ri, rs = SR.similar_reference(emb, kinds, K, 'dot')              # once per distinct query
    r = np.arange(TRIGGER_U) % kinds.size
    got = run_similar(emb, kinds[r], K, 'dot')
    assert_exact(got, (ri[r], rs[r]))


COS_CASES = [(1, 64, 2, 1), (7, 512, 17, 15), (7, 64, 18, 17), (10, 64, 65, 16), (10, 512, 66, 16), (256, 512, 17, 16), (64, 512, 14720, 17),
             (256, 64, 14720, 16), (100, 512, 14720, 4096), (10, 64, 14720, 16400)]


@pytest.mark.parametrize('K,E,N1,Q', COS_CASES)
def test_similar_exact_cosine(K, E, N1, Q):
    """16 entries of +-2^a per row: norms, inverse norms, their product and the score m / 16 are exact, at most 33 values: ties decide"""
    rng = np.random.default_rng(K * 11 + E + N1 + Q)
    emb = torch.from_numpy(SR.exact_cosine_table(rng, N1, E)).to(DEV)
    query = rng.integers(1, N1, size=Q)
    got = run_similar(emb, query, K, 'cos')
    assert_exact(got, SR.similar_reference(emb, query, K, 'cos'))
    listed = got[1][got[0] != 0]
    assert np.all(listed * 16 == np.round(listed * 16)) and np.unique(listed).size <= 33


@pytest.mark.parametrize('E', (64, 256))
def test_similar_dot_equals_topk_items_bit_for_bit(E):
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(E)
    N1, Q, K = 14720, 33, 100
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    query = rng.integers(1, N1, size=Q)
    got = run_similar(emb, query, K, 'dot')
    ptr, flat = csr([[int(q)] for q in query])
    ids = torch.empty(Q, K, dtype=torch.int32, device=DEV)
    sc = torch.empty(Q, K, dtype=torch.float32, device=DEV)
    L.topk_items(emb[torch.from_numpy(query).to(DEV)].contiguous(), emb, torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), K, ids, sc)
    torch.cuda.synchronize()
    assert_exact(got, (ids.cpu().numpy(), sc.cpu().numpy()))


@pytest.mark.parametrize('K,E', [(10, 64), (100, 128), (256, 64), (32, 256), (10, 512)])
def test_similar_random_tables_against_fp64(K, E):
    """Every returned score within b(q, i) of the fp64 cosine; every decided position (the restatement's scores at K + 1 depth separated from both
    neighbours by more than 2 max b) holds the restatement's id; at least 90 % of the positions are decided (the restatement alone gives 94 - 99 %
    on these cases: tests/test_similar_cpu.py)."""
    rng = np.random.default_rng(K + E)
    Q, N1 = 64, 14720
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    query = rng.integers(1, N1, size=Q)
    ids, sc = run_similar(emb, query, K, 'cos')
    s64 = SR.scores64(emb, torch.from_numpy(query), 'cos')[0].cpu().numpy()
    b = SR.cosine_bounds(emb, query)
    ri, rs = SR.similar_reference(emb, query, K + 1, 'cos')
    assert (ids != 0).all()
    rows = np.arange(Q)[:, None]
    err = np.abs(sc.astype(np.float64) - s64[rows, ids])
    print(f'K = {K}, E = {E}: largest |score - fp64| / b = {float((err / b[rows, ids]).max()):.3f}')
    assert np.all(err <= b[rows, ids])
    sure = SR.decided(rs, b.max(1))
    print(f'decided positions: {100 * sure.mean():.1f} %')
    assert sure.mean() >= 0.90
    np.testing.assert_array_equal(ids[sure], ri[:, :K][sure])


def test_similar_scores_are_symmetric_bit_for_bit():
    rng = np.random.default_rng(5)
    N1, E, K = 2049, 128, 256
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    for metric in ('cos', 'dot'):
        ids, sc = run_similar(emb, np.arange(1, N1), K, metric)
        bits = np.zeros((N1, N1), np.uint32)
        listed = np.zeros((N1, N1), bool)
        rows = np.arange(1, N1)[:, None]
        bits[rows, ids] = BITS(sc)
        listed[rows, ids] = True
        both = listed & listed.T
        assert both.sum() > N1                                                    # mutual neighbours exist
        np.testing.assert_array_equal(bits[both], bits.T[both])


def _rules_table():
    rng = np.random.default_rng(8)
    N1, E = 300, 64
    t = SR.exact_cosine_table(rng, N1, E)
    t[9], t[12] = t[5], t[5] * 4                                                  # duplicates of row 5 (one scaled: cosine 1 all the same)
    t[20] = 0
    t[21, 3] = np.nan
    t[22, 7] = np.inf
    return torch.from_numpy(t).to(DEV), N1


def test_similar_rules_self_duplicates_dead_rows_and_queries():
    emb, N1 = _rules_table()
    K = 12
    query = np.array([5, 9, 12, 20, 21, 22, 0, -1, N1, N1 + 5, 2 ** 31 - 1, 33, 33, 5])
    ids, sc = run_similar(emb, query, K, 'cos')
    assert_exact((ids, sc), SR.similar_reference(emb, query, K, 'cos'))
    for r, q in enumerate(query):
        assert q == 0 or q not in ids[r]                                           # self is never listed
        assert not set(ids[r]) & {20, 21, 22}                                      # zero, NaN and inf rows are no one's neighbour
    assert ids[0, :2].tolist() == [9, 12] and ids[1, :2].tolist() == [5, 12] and ids[2, :2].tolist() == [5, 9]
    assert (sc[:3, :2] == 1.0).all()                                               # duplicates first, at equal score, by id
    for r in range(3, 11):                                                         # dead rows and ids that are no item: pads only
        assert (ids[r] == 0).all() and np.isneginf(sc[r]).all(), r
    np.testing.assert_array_equal(ids[11], ids[12])                                # repeated query ids: equal rows
    np.testing.assert_array_equal(BITS(sc[11]), BITS(sc[12]))
    np.testing.assert_array_equal(ids[0], ids[13])
    # the dot metric on the finite rows: a zero query row scores 0 everywhere, the smallest ids
    fin = torch.nan_to_num(emb, nan=0.0, posinf=0.0)
    got = run_similar(fin, query, K, 'dot')
    assert_exact(got, SR.similar_reference(fin, query, K, 'dot'))
    assert got[0][3].tolist() == list(range(1, K + 1)) and (got[1][3] == 0).all()


def test_similar_candidates_and_floor():
    emb, N1 = _rules_table()
    rng = np.random.default_rng(9)
    K = 10
    cand = rng.random(N1) < 0.5
    cand[[5, 33]] = False                                                          # queries that are no candidates
    cand[9] = True
    query = np.array([5, 33, 9, 40, 41, 42, 250])
    cdev = torch.from_numpy(cand).to(DEV)
    for metric in ('cos', 'dot'):
        t = emb if metric == 'cos' else torch.nan_to_num(emb, nan=0.0, posinf=0.0)
        ids, sc = run_similar(t, query, K, metric, cand=cdev)
        assert_exact((ids, sc), SR.similar_reference(t, query, K, metric, cand=cand))
        assert cand[ids[ids != 0]].all() and (ids != 0).any(1).all()
        assert_exact(run_similar(t, query, K, metric, cand=cdev.view(torch.uint8)), (ids, sc))
    # the floor: the entries of the unfloored K = 256 list at or above it, cut to K
    full_i, full_s = run_similar(emb, query, 256, 'cos')
    for floor in (0.25, 0.0, -0.125, 1.0, 1.5, -float('inf')):
        ids, sc = run_similar(emb, query, K, 'cos', min_sim=floor)
        assert_exact((ids, sc), SR.similar_reference(emb, query, K, 'cos', min_sim=floor))
        for r in range(len(query)):
            keep = (full_i[r] != 0) & (full_s[r] >= floor)
            n = min(K, int(keep.sum()))
            assert ids[r, :n].tolist() == full_i[r][keep][:n].tolist() and (ids[r, n:] == 0).all() and np.isneginf(sc[r, n:]).all(), (floor, r)
    assert (run_similar(emb, query, K, 'cos', min_sim=1.5)[0] == 0).all()
    assert (run_similar(emb, query[:1], K, 'cos', min_sim=1.0)[0][0, :3] == [9, 12, 0]).all()


@pytest.mark.parametrize('E', (64, 128, 256, 512))
@pytest.mark.parametrize('N1', (1, 2, 17, 14720))
def test_row_inv_norms(N1, E):
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(N1 + E)
    x = (rng.standard_normal((N1, E)) * np.exp2(rng.integers(-20, 21, size=(N1, 1)))).astype(np.float32)
    got = L.row_inv_norms(torch.from_numpy(x).to(DEV)).cpu().numpy()
    ref = SR.inv_norms_reference(torch.from_numpy(x))
    assert got.dtype == np.float32 and got.shape == (N1,)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(ref)), float(np.abs(got - ref).max())      # within 1 fp32 ulp
    y = rng.integers(-8, 9, size=(N1, E)).astype(np.float32)                      # integer rows: the fp64 sum is exact, the result the same bits
    if N1 >= 17:
        y[3] = 0
        y[4, E - 1] = np.inf
        y[5, 0] = np.nan
        y[6, 1] = -np.inf
    out = torch.full((N1,), 7.0, device=DEV)
    assert L.row_inv_norms(torch.from_numpy(y).to(DEV), out) is out
    np.testing.assert_array_equal(BITS(out.cpu().numpy()), BITS(SR.inv_norms_reference(torch.from_numpy(y))))
    if N1 >= 17:
        assert (out[3:7] == 0).all() and (out[7:] > 0).all()


def test_similar_deterministic_and_grid_independent():
    rng = np.random.default_rng(4)
    Q, N1, E, K = 16400, 14720, 64, 10
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    query = rng.integers(1, N1, size=Q)
    a = run_similar(emb, query, K, 'cos')
    assert_exact(run_similar(emb, query, K, 'cos'), a)
    for r in (0, 12345, Q - 1):                                                   # alone: 1 workgroup x 32 item ranges + the merge; in the batch: 1 range
        i1, s1 = run_similar(emb, query[r:r + 1], K, 'cos')
        np.testing.assert_array_equal(i1[0], a[0][r])
        np.testing.assert_array_equal(BITS(s1[0]), BITS(a[1][r]))


def test_similar_argument_errors_launch_nothing():
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    Q, N1 = 16, 101
    emb = torch.randn(N1, 128, device=DEV)
    inv = torch.full((N1,), 7.0, device=DEV)
    query = torch.arange(1, Q + 1, dtype=torch.int32, device=DEV)
    ids = torch.full((Q, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((Q, 257), 7.0, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    f, g = lib.a4r_topk_similar, lib.a4r_row_inv_norms
    assert (f.restype, f.argtypes) == L.SIMILAR_SIGNATURES['a4r_topk_similar'] and (g.restype, g.argtypes) == L.SIMILAR_SIGNATURES['a4r_row_inv_norms']
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    inf = float('inf')
    # (emb offset, ws offset, min_sim, Q, N1, E, K)
    for eo, wo, floor, q, n1, E, K in ((0, 0, -inf, Q, N1, 128, 0), (0, 0, -inf, Q, N1, 128, 257), (0, 0, -inf, Q, N1, 96, 10), (4, 0, -inf, Q, N1, 64, 10),
                                       (0, 4, -inf, Q, N1, 64, 10), (0, 0, float('nan'), Q, N1, 64, 10), (0, 0, -inf, 0, N1, 64, 10), (0, 0, -inf, Q, 1, 64, 10)):
        for iv in (P(inv), None):
            assert f(None, P(emb, eo), iv, P(query), None, floor, P(ids), P(sc), P(ws, wo), q, n1, E, K) == -1, (eo, wo, floor, q, n1, E, K)
    for null in (1, 3, 6, 7, 8):
        a = [None, P(emb), P(inv), P(query), None, -inf, P(ids), P(sc), P(ws), Q, N1, 128, 10]
        a[null] = None
        assert f(*a) == -1, null
    for a in ((None, P(inv), N1, 128), (P(emb), None, N1, 128), (P(emb), P(inv), 0, 128), (P(emb), P(inv), N1, 96), (P(emb, 4), P(inv), N1, 64)):
        assert g(None, *a) == -1, a
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all()) and bool((inv == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ API level

class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _id_table():
    import test_id_tower_cpu as CPU
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    model, fx, _ = CPU.build('sasrec', compute_dtype='fp32')
    args = CPU.make_args(arch='sasrec', adapter_type='None')
    item_num = int(fx['item_num'])
    return get_itemId_embeddings(model.to(DEV), item_num, 256, args, 0), item_num


@pytest.mark.parametrize('metric', ('cos', 'dot'))
def test_similar_items_on_the_id_table_against_the_restatement(metric, monkeypatch):
    from adapter4rec_amd.data_utils.metrics import similar_items
    emb, item_num = _id_table()
    k = 7
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '25')                                # three batches
    ids, sc = similar_items(emb, k, metric=metric)
    assert ids.dtype == torch.long and tuple(ids.shape) == (item_num, k) == tuple(sc.shape) and ids.device == emb.device
    query = np.arange(1, item_num + 1)
    ri, rs = SR.similar_reference(emb, query, k + 1, metric)
    if metric == 'cos':
        b = SR.cosine_bounds(emb, query)
    else:
        t = emb.double()
        b = (emb.shape[1] * 2.0 ** -24 * (t[1:].abs() @ t.abs().t())).cpu().numpy()
    sure = SR.decided(rs, b.max(1))
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert sure.mean() > 0.9
    np.testing.assert_array_equal(ids[sure], ri[:, :k][sure])
    assert np.all((np.abs(sc - rs[:, :k]) <= b.max(1)[:, None])[sure])
    some = np.array([7, 3, 3, 60, 0, 99])
    i2, s2 = similar_items(emb, k, item_ids=some, metric=metric)
    np.testing.assert_array_equal(i2[:4].cpu().numpy(), ids[some[:4] - 1])
    assert (i2[4:] == 0).all() and torch.isneginf(s2[4:]).all()


def test_write_similar_items_round_trips(tmp_path):
    from adapter4rec_amd.data_utils.metrics import similar_items, write_similar_items
    emb, item_num = _id_table()
    emb = emb.clone()
    emb[11] = 0                                                                    # an item without any neighbour: no line
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    path, log = str(tmp_path / 'sim.tsv'), _Log()
    query = np.array([4, 11, 2, 60])
    assert write_similar_items(emb, 5, 16, names, path, item_ids=query, min_sim=0.05, Log_file=log) == path
    ids, sc = similar_items(emb, 5, item_ids=query, min_sim=0.05)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    assert [r[0] for r in rows] == ['N4', 'N2', 'N60'] and (ids[1] == 0).all()
    for r, row in zip((0, 2, 3), rows):
        keep = ids[r] != 0
        assert row[1].split(' ') == [f'N{i}' for i in ids[r][keep]]
        assert [np.float32(x) for x in row[2].split(' ')] == sc[r][keep].tolist()      # %.9g round-trips fp32
    assert len(log.lines) == 1 and log.lines[0].startswith('similar   top-5 lists of 4 items, 3 with a neighbour, mean best score ') and log.lines[0].endswith('-> ' + path)
