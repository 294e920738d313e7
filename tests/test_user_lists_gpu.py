"""a4r_topk_lists / a4r_eval_rank_lists on the MI355X (include/a4r_user_lists.h): exact lists and ranks on integer-valued tables at every list
length on either side of K, of the 64-key minimum sort and of A4R_LIST_MAX; the bits of the table sweep under a list that names every item;
max_len and the end of the CSR honoured; random tables against fp64; determinism and batch independence; more users than the grid holds;
argument errors; and recommend() / eval_model() with candidate_lists on a tiny ID model.

Integer-valued tables in [-2, 2] make every dot product an integer of magnitude <= 4 E <= 2048: exact in fp32 whatever the summation order, so
ids, score bits and ranks are compared exactly against the numpy restatement of tests/lists_ref.py, and ties are plentiful."""
import ctypes as C

import numpy as np
import pytest
import torch

import lists_ref as LR
from test_topk_gpu import excl_lists
from topk_ref import csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_topk(prec, emb, lists, excl, K, max_len=None, list_csr=None):
    """-> (ids, scores) as numpy; ``list_csr``: (ptr, flat) device tensors to use as they are instead of building them from ``lists``"""
    from adapter4rec_amd import _lib as L
    U = prec.shape[0]
    if list_csr is None:
        ptr, flat = LR.csr_tail(lists)                                            # nothing behind the last list
        list_csr = (dev(ptr), dev(flat))
    if max_len is None:
        max_len = max(len(x) for x in lists)
    xp, xf = csr(excl)
    ids = torch.full((U, K), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, K), 7.0, dtype=torch.float32, device=DEV)
    L.topk_lists(prec, emb, list_csr[0], list_csr[1], max_len, dev(xp), dev(xf), K, ids, sc)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def run_rank(prec, emb, target, lists, hist, max_len=None, list_csr=None):
    from adapter4rec_amd import _lib as L
    U = prec.shape[0]
    if list_csr is None:
        ptr, flat = LR.csr_tail(lists)
        list_csr = (dev(ptr), dev(flat))
    if max_len is None:
        max_len = max(len(x) for x in lists)
    hp, hf = csr(hist)
    rank = torch.full((U,), -7, dtype=torch.int32, device=DEV)
    L.eval_rank_lists(prec, emb, dev(np.asarray(target, np.int32)), list_csr[0], list_csr[1], max_len, dev(hp), dev(hf), rank)
    torch.cuda.synchronize()
    return rank.cpu().numpy()


def integer_tables(rng, U, N1, E):
    emb = rng.integers(-2, 3, size=(N1, E)).astype(np.float32)
    prec = rng.integers(-2, 3, size=(U, E)).astype(np.float32)
    return prec, emb


def assert_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------ 1: exact on integer tables
# every U, N1 and K of {1, 5, 17} x {2, 37, 4099} x {1, 10, 256} occurs, each beside two values of the other two
SHAPES = [(1, 2, 1), (5, 37, 10), (17, 4099, 256), (17, 2, 10), (5, 4099, 1), (1, 37, 256), (17, 37, 1), (1, 4099, 10), (5, 2, 256)]


def list_lengths(K):
    """on either side of K, of the 64-key minimum sort and of A4R_LIST_MAX; 600 and 1500 sort 1024 and 2048 keys, two and three steps a pass"""
    return [0, 1, K - 1, K, K + 1, 63, 64, 65, 4095, 4096, 600, 1500]


def exact_case(U, N1, K, E):
    rng = np.random.default_rng(1000 * E + 100 * U + N1 + K)
    prec, emb = integer_tables(rng, U, N1, E)
    lens = list_lengths(K)
    excl = excl_lists(rng, U, N1)                                                 # empty, 264 ids with repeats, short ones: in turn
    target = rng.integers(1, N1, size=U)
    lists = []
    for u in range(U):
        n = lens[(u + U + K) % len(lens)] if U < len(lens) else lens[u % len(lens)]
        x = rng.integers(-2, N1 + 3, size=n)                                      # id 0, negative ids, ids >= N1 among them
        if n >= 4:
            x[: n // 4] = x[n // 4: 2 * (n // 4)]                                # repeated ids
        lists.append(x)
    if U >= 5:
        # user 1: every listed item is excluded -> pad slots only, rank 1
        some = rng.integers(1, N1, size=40)
        lists[1], excl[1] = np.concatenate([some, some[:7], [0, -1, N1]]), np.concatenate([[0], some[::-1]])
        # user 2: the target is not in its list (its rank is the one it would have)
        lists[2] = np.where(lists[2] == target[2], 0, lists[2])
        # user 3: the target is listed (and, a repeat, listed twice)
        if len(lists[3]) >= 2:
            lists[3][0] = lists[3][-1] = target[3]
    return prec, emb, lists, excl, target


@pytest.mark.parametrize('E', [64, 128, 256, 512])
@pytest.mark.parametrize('U,N1,K', SHAPES, ids=lambda v: str(v))
def test_exact_on_integer_tables(U, N1, K, E):
    prec, emb, lists, excl, target = exact_case(U, N1, K, E)
    if U == 17:
        assert {len(x) for x in lists} >= set(list_lengths(K))                    # every length within the one call
    s64 = prec.astype(np.float64) @ emb.astype(np.float64).T
    ri, rs = LR.topk_lists_reference(s64, lists, excl, K)
    rr = LR.rank_lists_reference(s64, target, lists, excl)
    p, e = dev(prec), dev(emb)
    ids, sc = run_topk(p, e, lists, excl, K, max_len=4096)
    rank = run_rank(p, e, target, lists, excl, max_len=4096)
    np.testing.assert_array_equal(ids, ri)
    assert_bits(sc, rs)
    np.testing.assert_array_equal(rank, rr)
    if U >= 5:
        assert (ids[1] == 0).all() and np.isneginf(sc[1]).all() and rank[1] == 1
        assert target[2] not in lists[2]
    for u in range(U):                                                            # a repeated id is returned once; pad slots only behind the items
        real = ids[u][ids[u] != 0]
        assert len(set(real.tolist())) == real.size and (ids[u][real.size:] == 0).all()


# ------------------------------------------------------------------ 2: a list that names every item gives the table sweep
@pytest.mark.parametrize('E', [64, 128, 256, 512])
def test_full_list_equals_the_table_sweep(E):
    from adapter4rec_amd import _lib as L
    U, N1, K = 17, 4097, 256
    rng = np.random.default_rng(200 + E)
    prec, emb = integer_tables(rng, U, N1, E)
    excl = excl_lists(rng, U, N1)
    target = rng.integers(1, N1, size=U)
    lists = [np.arange(1, N1)] * U
    p, e = dev(prec), dev(emb)
    ids, sc = run_topk(p, e, lists, excl, K)
    rank = run_rank(p, e, target, lists, excl)
    xp, xf = csr(excl)
    xp, xf = dev(xp), dev(xf)
    ids0 = torch.empty(U, K, dtype=torch.int32, device=DEV)
    sc0 = torch.empty(U, K, dtype=torch.float32, device=DEV)
    rank0 = torch.zeros(U, dtype=torch.int32, device=DEV)
    L.topk_items(p, e, xp, xf, K, ids0, sc0)
    L.eval_rank(p, e, dev(target.astype(np.int32)), xp, xf, rank0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ids, ids0.cpu().numpy())
    assert_bits(sc, sc0.cpu().numpy())
    np.testing.assert_array_equal(rank, rank0.cpu().numpy())
    assert (rank > 1).any()


# ------------------------------------------------------------------ 3: max_len, negative lengths and the end of the CSR
def test_max_len_is_honoured_and_nothing_behind_the_lists_is_read():
    U, N1, K, E = 9, 4099, 10, 128
    rng = np.random.default_rng(33)
    prec, emb = integer_tables(rng, U, N1, E)
    best = 7                                                                      # the best item of every user: whoever reads it, lists it first
    prec[:] = prec[0]
    emb[best] = np.where(prec[0] >= 0, 2, -2)                                     # 2 sum |prec|: no other row reaches it
    lens = [300, 100, 101, 99, 0, 64, 65, 257, 180]
    lists = [np.where((x := rng.integers(1, N1, size=n)) == best, 1, x) for n in lens]
    for u in (0, 2, 7):
        lists[u][100] = best                                                      # right behind max_len = 100
    lists[3][98] = best                                                           # inside it
    excl = [[] for _ in range(U)]
    target = rng.integers(1, N1, size=U)
    s64 = prec.astype(np.float64) @ emb.astype(np.float64).T
    assert (s64.argmax(1) == best).all() and (np.sort(s64, 1)[:, -2] < s64[:, best]).all()
    p, e = dev(prec), dev(emb)
    for max_len in (100, 64, 0):
        ri, rs = LR.topk_lists_reference(s64, lists, excl, K, max_len)
        rr = LR.rank_lists_reference(s64, target, lists, excl, max_len)
        ids, sc = run_topk(p, e, lists, excl, K, max_len=max_len)                 # the CSR ends with its allocation: csr_tail leaves no spare entry
        np.testing.assert_array_equal(ids, ri)
        assert_bits(sc, rs)
        np.testing.assert_array_equal(run_rank(p, e, target, lists, excl, max_len=max_len), rr)
    assert not (ri != 0).any()                                                    # max_len = 0: pad slots only
    ids, _ = run_topk(p, e, lists, excl, K, max_len=100)
    assert best not in ids[[0, 2, 7]] and ids[3, 0] == best
    # the same lists inside a larger buffer, the best item standing right behind the last list: it is never read
    ptr, flat = LR.csr_tail(lists)
    big = np.full(flat.size + 4096, best, np.int32)
    big[:flat.size] = flat
    big_d = dev(big)
    ids2, sc2 = run_topk(p, e, lists, excl, K, max_len=300, list_csr=(dev(ptr), big_d[:flat.size]))
    ri, rs = LR.topk_lists_reference(s64, lists, excl, K, 300)
    np.testing.assert_array_equal(ids2, ri)
    assert best not in ids2[[1, 4, 5, 6, 8]]
    # a negative length counts as 0: user 1's list ends in front of where it starts
    ptr2 = ptr.copy()
    ptr2[2] = ptr2[1] - 3
    lists2 = [flat[ptr2[u]:ptr2[u + 1]] if ptr2[u + 1] >= ptr2[u] else [] for u in range(U)]
    assert len(lists2[1]) == 0 and len(lists2[2]) == lens[2] + lens[1] + 3
    ids3, sc3 = run_topk(p, e, lists2, excl, K, max_len=300, list_csr=(dev(ptr2), dev(flat)))
    ri, rs = LR.topk_lists_reference(s64, lists2, excl, K, 300)
    np.testing.assert_array_equal(ids3, ri)
    assert (ids3[1] == 0).all()
    np.testing.assert_array_equal(run_rank(p, e, target, lists2, excl, max_len=300, list_csr=(dev(ptr2), dev(flat))),
                                  LR.rank_lists_reference(s64, target, lists2, excl, 300))


# ------------------------------------------------------------------ 4: random tables against fp64
_RANDOM = {}


def random_run(E):
    """the random case of lists_ref on the device, once per E"""
    if E not in _RANDOM:
        prec, emb, lists, excl, target = LR.random_case(E)
        p, e = dev(prec), dev(emb)
        ids, sc = run_topk(p, e, lists, excl, LR.RANDOM_CASE['K'])
        rank = run_rank(p, e, target, lists, excl)
        _RANDOM[E] = (prec, emb, lists, excl, target, p, e, ids, sc, rank)
    return _RANDOM[E]


@pytest.mark.parametrize('E', LR.RANDOM_E)
def test_random_tables_against_fp64(E):
    """Standard-normal tables, U = 48, N1 = 4099, K = 10, list lengths 0 .. 4096 (lists_ref.random_case): every returned score within the fp32
    summation bound E * 2^-24 * sum |a b| (the user's maximum) of the fp64 score of its item, every position the gap rule makes sure equal to the
    fp64 list's -- at least 95 % of the item positions (asserted here and, from the fp64 reference alone, in tests/test_user_lists_cpu.py) --
    every listed item from the user's list and outside its exclusion list, and every rank between the counts the bound allows."""
    prec, emb, lists, excl, target, p, e, ids, sc, rank = random_run(E)
    K, N1 = LR.RANDOM_CASE['K'], emb.shape[0]
    s64, bound, ri, rs, sure, real = LR.fp64_reference(prec, emb, lists, excl, K)
    assert sure.sum() / real.sum() >= 0.95
    worst = 0.0
    for u in range(prec.shape[0]):
        b = bound[u].max()
        items = np.setdiff1d(LR.listed(lists[u], N1), LR.listed(excl[u][:264], N1, 264))
        n = min(K, items.size)
        assert (ids[u, :n] != 0).all() and (ids[u, n:] == 0).all() and np.isneginf(sc[u, n:]).all(), u      # as many items as the reference, then pads
        assert set(ids[u, :n].tolist()) <= set(items.tolist()) and len(set(ids[u, :n].tolist())) == n, u
        err = np.abs(sc[u, :n].astype(np.float64) - s64[u, ids[u, :n]])
        worst = max(worst, float((err / b).max()) if n else 0.0)
        assert (err <= b).all(), (u, err.max(), b)
        np.testing.assert_array_equal(ids[u][sure[u]], ri[u][:K][sure[u]])
        s, t = s64[u, items], s64[u, target[u]]
        assert 1 + int((s > t + b).sum()) <= rank[u] <= 1 + int((s >= t - b).sum()), (u, rank[u])
    print(f'E = {E}: largest score error {worst:.3f} of the bound')
    assert (rank > 1).any()


# ------------------------------------------------------------------ 5: determinism
def test_deterministic_and_independent_of_the_batch():
    prec, emb, lists, excl, target, p, e, ids, sc, rank = random_run(128)
    K = LR.RANDOM_CASE['K']
    ids2, sc2 = run_topk(p, e, lists, excl, K)
    np.testing.assert_array_equal(ids, ids2)
    assert_bits(sc, sc2)
    np.testing.assert_array_equal(rank, run_rank(p, e, target, lists, excl))
    for a, b in ((0, 1), (7, 23), (36, 48)):                                      # users [a, b) alone: the slice of the full call
        i3, s3 = run_topk(p[a:b].contiguous(), e, lists[a:b], excl[a:b], K)
        np.testing.assert_array_equal(i3, ids[a:b])
        assert_bits(s3, sc[a:b])
        np.testing.assert_array_equal(run_rank(p[a:b].contiguous(), e, target[a:b], lists[a:b], excl[a:b]), rank[a:b])
    # the same item at another place of another user's list has the same score bits: scores are a pure function of (user, item)
    both = prec[[3, 3]].copy()
    l0 = np.asarray(lists[11][:500])
    i4, s4 = run_topk(dev(both), e, [l0, np.concatenate([np.zeros(37, np.int64), l0[::-1]])], [[], []], K)
    np.testing.assert_array_equal(i4[0], i4[1])
    assert_bits(s4[0], s4[1])


# ------------------------------------------------------------------ more users than workgroups in the grid
def test_more_users_than_the_grid_holds():
    U, N1, E, K = 65536 + 5, 37, 64, 2
    rng = np.random.default_rng(66)
    prec, emb = integer_tables(rng, U, N1, E)
    a = rng.integers(1, N1, size=U)
    b = 1 + (a - 1 + rng.integers(1, N1 - 1, size=U)) % (N1 - 1)                  # another item
    assert (a != b).all()
    target = rng.integers(1, N1, size=U)
    flat = np.stack([a, b], 1).reshape(-1).astype(np.int32)
    ptr = (2 * np.arange(U + 1)).astype(np.int32)
    csr_d = (dev(ptr), dev(flat))
    none = [[]] * U
    p, e = dev(prec), dev(emb)
    ids, sc = run_topk(p, e, None, none, K, max_len=2, list_csr=csr_d)
    rank = run_rank(p, e, target, None, none, max_len=2, list_csr=csr_d)
    sa = np.einsum('ue,ue->u', prec, emb[a])
    sb = np.einsum('ue,ue->u', prec, emb[b])
    st = np.einsum('ue,ue->u', prec, emb[target])
    first_a = (sa > sb) | ((sa == sb) & (a < b))
    np.testing.assert_array_equal(ids, np.where(first_a[:, None], np.stack([a, b], 1), np.stack([b, a], 1)))
    want = np.where(first_a[:, None], np.stack([sa, sb], 1), np.stack([sb, sa], 1)).astype(np.float32)
    want[want == 0] = 0.0
    assert_bits(sc, want)
    np.testing.assert_array_equal(rank, 1 + (sa > st).astype(np.int64) + (sb > st))


# ------------------------------------------------------------------ argument errors
def test_argument_errors_launch_nothing():
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    U, N1, k = 16, 101, 10
    emb = torch.randn(N1, 128, device=DEV)
    prec = torch.randn(U, 128, device=DEV)
    ptr = torch.zeros(U + 1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    tgt = torch.ones(U, dtype=torch.int32, device=DEV)
    rank = torch.full((U,), 7, dtype=torch.int32, device=DEV)
    ids = torch.full((U, k), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, k), 7.0, device=DEV)
    ft, fr = lib.a4r_topk_lists, lib.a4r_eval_rank_lists
    assert (ft.restype, ft.argtypes) == L.USER_LISTS_SIGNATURES['a4r_topk_lists']                # installed by lib()
    assert (fr.restype, fr.argtypes) == L.USER_LISTS_SIGNATURES['a4r_eval_rank_lists']
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for E, K, ml in ((96, 10, 5), (128, 0, 5), (128, 257, 5), (128, 10, -1), (128, 10, 4097)):
        assert ft(None, P(prec), P(emb), P(ptr), P(idx), P(ptr), P(idx), P(ids), P(sc), U, N1, E, K, ml) == -1, (E, K, ml)
    assert ft(None, P(prec, 4), P(emb), P(ptr), P(idx), P(ptr), P(idx), P(ids), P(sc), U, N1, 64, k, 5) == -1
    assert ft(None, P(prec), P(emb), P(ptr), None, P(ptr), P(idx), P(ids), P(sc), U, N1, 128, k, 5) == -1
    for E, ml in ((96, 5), (128, -1), (128, 4097)):
        assert fr(None, P(prec), P(emb), P(tgt), P(ptr), P(idx), P(ptr), P(idx), P(rank), U, N1, E, ml) == -1, (E, ml)
    assert fr(None, P(prec), P(emb, 8), P(tgt), P(ptr), P(idx), P(ptr), P(idx), P(rank), U, N1, 128, 5) == -1
    for bad in (dict(k=0), dict(k=257), dict(max_len=4097), dict(list_ptr=ptr[:-1].contiguous()), dict(list_idx=idx.long()), dict(list_ptr=ptr.cpu())):
        kw = dict(dict(prec=prec, item_emb=emb, list_ptr=ptr, list_idx=idx, max_len=0, excl_ptr=ptr, excl_idx=idx, k=k, ids=ids, scores=sc), **bad)
        with pytest.raises((ValueError, RuntimeError)):
            L.topk_lists(**kw)
    with pytest.raises(ValueError, match='max_len'):
        L.eval_rank_lists(prec, emb, tgt, ptr, idx, 5000, ptr, idx, rank)
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all()) and bool((rank == 7).all())
    # served: every list empty
    L.topk_lists(prec, emb, ptr, idx[:0], 0, ptr, idx[:0], k, ids, sc)
    L.eval_rank_lists(prec, emb, tgt, ptr, idx[:0], 0, ptr, idx[:0], rank)
    torch.cuda.synchronize()
    assert bool((ids == 0).all()) and bool(torch.isneginf(sc).all()) and bool((rank == 1).all())


# ------------------------------------------------------------------ 6: API level
def test_recommend_and_eval_model_with_candidate_lists_on_an_id_model(monkeypatch):
    """recommend(..., candidate_lists=) and eval_model(..., candidate_lists=) on the small ID model, against the restatement on the fp64 product
    of the vectors the user tower handed the kernels: scores within the summation bound, sure positions equal, ranks within the interval the
    bound allows, the means over the users who have a list -- and HR@10 counted from recommend's own lists."""
    from test_topk_gpu import _id_model
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import eval_model, eval_ranks, recommend
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    N1, E = emb.shape
    rng = np.random.default_rng(9)
    U, k = 300, 10
    eval_seq, hist = {}, {}
    for u in range(U):
        s = [int(x) for x in rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False)]
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    target = np.array([eval_seq[u][-1] for u in range(U)])
    lists = {}
    for u in range(U):
        if u % 4 == 3:
            continue                                                              # no list
        x = rng.integers(0, item_num + 2, size=int(rng.integers(0, 120)))
        if u % 2 == 0 and x.size:
            x[0] = target[u]                                                      # the held-out item among its sampled negatives
        lists[u] = x
    has = np.array([u in lists for u in range(U)])
    seen = {}
    real_topk, real_rank = L.topk_lists, L.eval_rank_lists
    monkeypatch.setattr(L, 'topk_lists', lambda prec, *a: (seen.setdefault('topk', []).append(prec.clone()), real_topk(prec, *a))[1], raising=False)
    monkeypatch.setattr(L, 'eval_rank_lists', lambda prec, *a: (seen.setdefault('rank', []).append(prec.clone()), real_rank(prec, *a))[1], raising=False)
    for name in ('topk_items', 'eval_rank'):
        monkeypatch.setattr(L, name, lambda *a, **k: pytest.fail('a whole-table call under candidate lists'))

    class Log:
        lines = []

        def info(self, msg):
            self.lines.append(str(msg))
    hr = eval_model(model, hist, eval_seq, emb, 256, args, item_num, Log(), 'test', 0, candidate_lists=lists)
    assert f'test_candidate_lists   {int(has.sum())} of {U} users' in Log.lines
    ranks = eval_ranks(model, hist, eval_seq, emb, 256, args, list(range(U)), candidate_lists=lists).cpu().numpy()
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    ids, sc = recommend(model, seqs, emb, k, args, exclude=hist, candidate_lists=lists)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    e64 = emb.double().cpu().numpy()
    full = [lists.get(u, []) for u in range(U)]
    hl = [hist[u].numpy() for u in range(U)]
    p_rank, p_topk = torch.cat(seen['rank'][-1:]).double().cpu().numpy(), torch.cat(seen['topk']).double().cpu().numpy()
    assert p_rank.shape == p_topk.shape == (U, E)
    for pv, what in ((p_rank, 'rank'), (p_topk, 'topk')):
        s64 = pv @ e64.T
        bound = E * 2.0 ** -24 * (np.abs(pv) @ np.abs(e64).T)
        if what == 'rank':
            hits = 0
            for u in range(U):
                b = bound[u].max()
                items = np.setdiff1d(LR.listed(full[u], N1), LR.listed(hl[u], N1, 264))
                s, t = s64[u, items], s64[u, target[u]]
                assert 1 + int((s > t + b).sum()) <= ranks[u] <= 1 + int((s >= t - b).sum()), u
                hits += int(has[u] and ranks[u] <= 10)
            assert abs(hr - hits / has.sum()) < 1e-6 and (ranks[~has] == 1).all() and (ranks > 10).any()
        else:
            ri, rs = LR.topk_lists_reference(s64, full, hl, k + 1)
            for u in range(U):
                b = bound[u].max()
                n = int((ri[u, :k] != 0).sum())
                assert (ids[u, :n] != 0).all() and (ids[u, n:] == 0).all(), u
                assert (np.abs(sc[u, :n] - s64[u, ids[u, :n]]) <= b).all(), u
                with np.errstate(invalid='ignore'):
                    sep = np.concatenate([[True], -np.diff(rs[u]) > b])
                sure = sep[:k] & sep[1:k + 1] & (ri[u, :k] != 0)
                np.testing.assert_array_equal(ids[u][sure], ri[u, :k][sure])
                assert set(ids[u, :n].tolist()) <= set(int(x) for x in full[u]) - set(hl[u].tolist()), u
    # rank and top-K agree: a listed, unseen target with rank r <= k stands at position r of the user's list
    for u in np.flatnonzero(has & (ranks <= k)):
        if target[u] in set(int(x) for x in lists[u]):
            assert ids[u, ranks[u] - 1] == target[u], u
    with pytest.raises(ValueError, match='cannot be combined'):
        recommend(model, seqs, emb, k, args, exclude=hist, candidate_lists=lists, candidates=np.ones(item_num + 1, bool))
    with pytest.raises(ValueError, match='no user'):
        eval_model(model, hist, eval_seq, emb, 256, args, item_num, Log(), 'test', 0, candidate_lists={})
