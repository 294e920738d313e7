"""a4r_eval_rank_cand / a4r_topk_items_cand on the MI355X (include/a4r_candidates.h): exact ranks and lists on integer-valued tables under every kind
of candidate set, the bits of the unmasked entries under an all-ones set, rank and top-K held against each other, determinism across grids, one
random table against fp64, argument errors, the torch ops, and recommend() / eval_model() with a mask on a tiny ID model.

Integer-valued tables in [-8, 8] make every score an integer below 2^24: exact in fp32 whatever the summation order, so ids, ranks and score
bits are compared exactly, at every position.  The oracle is formed on the device (a masked score matrix, a stable sort); wherever the shape
allows (U <= 64) the numpy restatement of tests/cand_ref.py is held against the kernels as well."""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

import cand_ref as CR
from test_topk_gpu import excl_lists
from topk_ref import MAX_EXCL, csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(1, 64, 2, 1), (7, 128, 17, 15), (10, 64, 14720, 16), (256, 512, 17, 16), (64, 256, 65537, 17), (100, 64, 500000, 16), (10, 128, 65537, 4096)]
MASKS = ['ones', 'zeros', 'item1', 'last', 'k_minus_1', 'half', 'sparse', 'no_targets', 'pad_entry']


def _pairs():
    """every shape under the 0.5 mask, every other kind of mask on two shapes (walking the shape list, so every shape sees several kinds)"""
    out = [(s, 'half') for s in SHAPES]
    j = 0
    for m in MASKS:
        if m == 'half':
            continue
        for _ in range(2):
            out.append((SHAPES[j % len(SHAPES)], m))
            j += 1
    return out


_INPUTS = {}


def inputs(shape):
    """The tables, lists and targets of a shape, built once: duplicated table rows (ties by id), all-zero users (every score 0), lists with 0 ids,
    264 ids with repeats, pad and out-of-range ids; every fourth user's target sits inside its own list where that list names an item."""
    if shape not in _INPUTS:
        K, E, N1, U = shape
        rng = np.random.default_rng(K * 7 + E + N1 + U)
        emb = torch.from_numpy(rng.integers(-8, 9, size=(N1, E)).astype(np.float32))
        if N1 > 8:
            src = rng.integers(1, N1, size=N1 // 8)
            emb[rng.integers(1, N1, size=N1 // 8)] = emb[src]
        prec = torch.from_numpy(rng.integers(-8, 9, size=(U, E)).astype(np.float32))
        prec[::5] = 0.0
        lists = excl_lists(rng, U, N1)
        target = rng.integers(1, N1, size=U)
        for u in range(1, U, 4):
            ok = lists[u][(lists[u] > 0) & (lists[u] < N1)]
            if ok.size:
                target[u] = ok[0]
        ptr, flat = csr(lists)
        _INPUTS[shape] = dict(prec=prec.to(DEV), emb=emb.to(DEV), lists=lists, target=target, ptr=torch.from_numpy(ptr).to(DEV),
                              flat=torch.from_numpy(flat).to(DEV), target32=torch.from_numpy(target.astype(np.int32)).to(DEV))
    return _INPUTS[shape]


def make_mask(kind, shape, target, seed=0):
    K, E, N1, U = shape
    rng = np.random.default_rng(1000 + seed + N1 + K)
    m = np.zeros(N1, np.uint8)
    if kind == 'ones':
        m[:] = 1
    elif kind == 'item1':
        m[1] = 1
    elif kind == 'last':
        m[N1 - 1] = 1
    elif kind == 'k_minus_1':
        n = min(K - 1, N1 - 1)
        m[rng.choice(np.arange(1, N1), size=n, replace=False)] = 1
        assert int(m.sum()) == n
    elif kind in ('half', 'pad_entry'):
        m[:] = rng.random(N1) < 0.5
    elif kind == 'sparse':
        m[:] = rng.random(N1) < 0.01
    elif kind == 'no_targets':
        m[:] = rng.random(N1) < 0.5
        m[target] = 0
    else:
        assert kind == 'zeros'
    m[m != 0] = rng.integers(1, 256, size=int((m != 0).sum()))                  # any non-zero byte marks a candidate
    return m


def run_masked(d, cand, K):
    from adapter4rec_amd import _lib as L
    U = d['prec'].shape[0]
    c = cand if isinstance(cand, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cand)).to(DEV)
    rank = torch.zeros(U, dtype=torch.int32, device=DEV)
    ids = torch.empty(U, K, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, K, dtype=torch.float32, device=DEV)
    L.eval_rank_cand(d['prec'], d['emb'], d['target32'], d['ptr'], d['flat'], c, rank)
    L.topk_items_cand(d['prec'], d['emb'], d['ptr'], d['flat'], c, K, ids, sc)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy()


def run_unmasked(d, K):
    from adapter4rec_amd import _lib as L
    U = d['prec'].shape[0]
    rank = torch.zeros(U, dtype=torch.int32, device=DEV)
    ids = torch.empty(U, K, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, K, dtype=torch.float32, device=DEV)
    L.eval_rank(d['prec'], d['emb'], d['target32'], d['ptr'], d['flat'], rank)
    L.topk_items(d['prec'], d['emb'], d['ptr'], d['flat'], K, ids, sc)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), ids.cpu().numpy(), sc.cpu().numpy()


def device_oracle(d, cand, K):
    """Exact scores (the fp64 product of integer tables, every value an integer below 2^24), the items outside the candidate set, the pad row and
    the user's list struck out, a count above the target's score and a stable descending sort -> (ranks, ids, scores)."""
    prec, emb, lists, target = d['prec'], d['emb'], d['lists'], d['target']
    U, N1 = prec.shape[0], emb.shape[0]
    c = torch.from_numpy(np.asarray(cand) != 0).to(DEV)
    ranks = np.zeros(U, np.int64)
    ids = np.zeros((U, K), np.int64)
    out = np.full((U, K), -np.inf, np.float32)
    emb64 = emb.double()
    for a in range(0, U, 512):
        b = min(a + 512, U)
        s = (prec[a:b].double() @ emb64.t()).float()
        allow = c[None, :].repeat(b - a, 1)
        allow[:, 0] = False
        rows, cols = [], []
        for u in range(a, b):
            x = np.asarray(list(lists[u])[:MAX_EXCL], np.int64).reshape(-1)
            x = x[(x > 0) & (x < N1)]
            rows.append(np.full(x.size, u - a, np.int64))
            cols.append(x)
        allow[torch.from_numpy(np.concatenate(rows)).to(DEV), torch.from_numpy(np.concatenate(cols)).to(DEV)] = False
        ts = s[torch.arange(b - a, device=DEV), torch.from_numpy(target[a:b]).to(DEV)]
        ranks[a:b] = 1 + ((s > ts[:, None]) & allow).sum(1).cpu().numpy()
        s = torch.where(allow, s, torch.full_like(s, -float('inf')))
        v, i = torch.sort(s, dim=1, descending=True, stable=True)              # stable: equal scores keep ascending ids
        n = min(K, N1)
        v, i = v[:, :n].cpu().numpy(), i[:, :n].cpu().numpy()
        i = np.where(np.isfinite(v), i, 0)
        ids[a:b, :n], out[a:b, :n] = i, v
    out[out == 0] = 0.0
    return ranks, ids, out


def check_exact(d, cand, K, got):
    rank, ids, sc = got
    wr, wi, ws = device_oracle(d, cand, K)
    np.testing.assert_array_equal(rank, wr)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(sc.view(np.uint32), ws.view(np.uint32))
    U = d['prec'].shape[0]
    if U <= 64:                                                                 # the numpy restatement, where [U, N1] fp64 on the host is small
        s64 = (d['prec'].double() @ d['emb'].double().t()).cpu().numpy()
        np.testing.assert_array_equal(rank, CR.rank_cand_reference(s64, d['target'], d['lists'], cand))
        ri, rs = CR.topk_cand_reference(s64, d['lists'], cand, K)
        np.testing.assert_array_equal(ids, ri)
        np.testing.assert_array_equal(sc.view(np.uint32), rs.astype(np.float32).view(np.uint32))
    return wr, wi


@pytest.mark.parametrize('shape,kind', _pairs(), ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_exact_on_integer_tables(shape, kind):
    K, E, N1, U = shape
    d = inputs(shape)
    cand = make_mask(kind, shape, d['target'])
    got = run_masked(d, cand, K)
    wr, wi = check_exact(d, cand, K, got)
    c = cand != 0
    c[0] = False
    assert c[wi[wi != 0]].all()                                                 # the oracle's own lists hold candidates only
    if kind == 'zeros':
        assert (got[0] == 1).all() and (got[1] == 0).all() and np.isinf(got[2]).all()
    if kind in ('item1', 'last'):
        assert (got[1][:, 1:] == 0).all() and set(np.unique(got[1])) <= {0, 1 if kind == 'item1' else N1 - 1}
    if kind == 'k_minus_1':
        assert (got[1][:, K - 1:] == 0).all()                                   # one slot short at least: padded
    if kind == 'no_targets':
        assert not c[d['target']].any()                                         # ranked as if they were candidates, by the oracle above
    if kind == 'pad_entry':                                                     # cand[0] set and cleared: no difference
        a, b = cand.copy(), cand.copy()
        a[0], b[0] = 1, 0
        ga, gb = run_masked(d, a, K), run_masked(d, b, K)
        for x, y, z in zip(ga, gb, got):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
            np.testing.assert_array_equal(x.view(np.uint32), z.view(np.uint32))
    if kind == 'half' and U >= 15 and N1 > 100:
        # the lists hold history ids that are no candidates (nothing to take back twice) and targets inside their own history
        hist_non = sum(int((~c[x[(x > 0) & (x < N1)]]).sum()) for x in d['lists'])
        inside = sum(int(d['target'][u] in set(d['lists'][u].tolist())) for u in range(U))
        assert hist_non > 0 and inside > 0


def test_bool_masks_are_masks_as_they_stand():
    shape = SHAPES[2]
    d = inputs(shape)
    cand = make_mask('half', shape, d['target'])
    a = run_masked(d, cand, shape[0])
    b = run_masked(d, torch.from_numpy(cand != 0).to(DEV), shape[0])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def _normal_case(U, N1, E, seed):
    rng = np.random.default_rng(seed)
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    tgt = rng.integers(1, N1, size=U)
    # users pointed at their targets so that many targets rank inside a list
    prec = (emb[torch.from_numpy(tgt).to(DEV)] * 0.3 + torch.from_numpy(rng.standard_normal((U, E)).astype(np.float32)).to(DEV)).contiguous()
    return rng, emb, prec, tgt


def _device_inputs(prec, emb, lists, tgt):
    ptr, flat = csr(lists)
    return dict(prec=prec, emb=emb, lists=lists, target=tgt, ptr=torch.from_numpy(ptr).to(DEV), flat=torch.from_numpy(flat).to(DEV),
                target32=torch.from_numpy(tgt.astype(np.int32)).to(DEV))


def test_all_ones_mask_gives_the_unmasked_bits():
    U, N1, E, K = 4096, 65537, 64, 100
    rng, emb, prec, tgt = _normal_case(U, N1, E, 21)
    d = _device_inputs(prec, emb, excl_lists(rng, U, N1), tgt)
    a = run_masked(d, np.ones(N1, np.uint8), K)
    b = run_unmasked(d, K)
    for x, y in zip(a, b):                                                      # ranks, ids and scores as uint32
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (a[0] > 1).any() and (a[0] <= K).any()


def test_topk_agrees_with_rank_under_one_mask():
    U, N1, E, K = 4096, 65537, 64, 100
    rng, emb, prec, tgt = _normal_case(U, N1, E, 22)
    hist = []
    for u in range(U):
        h = rng.integers(1, N1, size=int(rng.integers(1, 30)))
        hist.append(h[h != tgt[u]])
    cand = (rng.random(N1) < 0.5).astype(np.uint8)
    rank, ids, sc = run_masked(_device_inputs(prec, emb, hist, tgt), cand, K)
    inside = outside = 0
    for u in range(U):
        r = int(rank[u])
        if not cand[tgt[u]]:                                                    # no candidate: ranked, never listed
            assert tgt[u] not in ids[u], u
            outside += 1
        elif r <= K:
            inside += 1
            assert ids[u, r - 1] == tgt[u], (u, r)
            assert int((sc[u] > sc[u, r - 1]).sum()) == r - 1, u
        else:
            assert tgt[u] not in ids[u], u
    assert inside > U // 16 and outside > U // 4, (inside, outside)
    assert cand[ids[ids != 0]].all()


def test_deterministic_and_grid_independent():
    U, N1, E, K = 32768, 65537, 64, 100
    rng, emb, prec, tgt = _normal_case(U, N1, E, 23)
    lists = excl_lists(rng, U, N1)
    cand = (rng.random(N1) < 0.5).astype(np.uint8)
    d = _device_inputs(prec, emb, lists, tgt)
    a = run_masked(d, cand, K)
    b = run_masked(d, cand, K)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    for u in (0, 12345, U - 1):                                                 # alone: 1 workgroup x 32 item ranges + the merge; in the batch: 1 range
        one = run_masked(_device_inputs(prec[u:u + 1].contiguous(), emb, [lists[u]], tgt[u:u + 1]), cand, K)
        for x, y in zip(one, a):
            np.testing.assert_array_equal(x[0].view(np.uint32), y[u].view(np.uint32))


def test_random_tables_against_fp64():
    """Standard-normal tables, U = 64, N1 = 65537, E = 64, K = 10, mask at 0.5 (cand_ref.random_case): every returned score within the fp32
    summation bound E * 2^-24 * sum |a b| of the fp64 score of its item, every position the gap rule makes sure equal to the fp64 list's -- at
    least 95 % of them (asserted here and, from the fp64 reference alone, in tests/test_candidates_cpu.py) -- every listed item a candidate
    outside the user's list, and every rank between the counts the bound allows."""
    prec, emb, cand, lists, target = CR.random_case()
    K = CR.RANDOM_CASE['K']
    s64, bound, ri, rs, sure = CR.fp64_reference(prec, emb, cand, lists, K)
    assert sure.mean() >= 0.95, sure.mean()
    d = _device_inputs(torch.from_numpy(prec).to(DEV), torch.from_numpy(emb).to(DEV), lists, target)
    rank, ids, sc = run_masked(d, cand, K)
    N1 = emb.shape[0]
    for u in range(prec.shape[0]):
        assert (ids[u] != 0).all() and (cand[ids[u]] != 0).all(), u
        assert not set(ids[u].tolist()) & set(int(x) for x in lists[u] if 0 < x < N1), u
        assert np.all(np.abs(sc[u] - s64[u, ids[u]]) <= bound[u, ids[u]]), u
        np.testing.assert_array_equal(ids[u][sure[u]], ri[u][:K][sure[u]])
        ok = cand != 0
        ok[0] = False
        x = np.asarray(lists[u], np.int64)
        ok[x[(x > 0) & (x < N1)]] = False
        ok[target[u]] = False
        diff, b2 = s64[u, ok] - s64[u, target[u]], bound[u, ok] + bound[u, target[u]]
        assert 1 + int((diff > b2).sum()) <= rank[u] <= 1 + int((diff > -b2).sum()), u


def test_argument_errors_launch_nothing():
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    U, N1 = 16, 101
    emb = torch.randn(N1, 128, device=DEV)
    prec = torch.randn(U, 128, device=DEV)
    ptr = torch.zeros(U + 1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    tgt = torch.ones(U, dtype=torch.int32, device=DEV)
    cand = torch.ones(N1, dtype=torch.uint8, device=DEV)
    rank = torch.full((U,), 7, dtype=torch.int32, device=DEV)
    ids = torch.full((U, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, 257), 7.0, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    fr, ft = lib.a4r_eval_rank_cand, lib.a4r_topk_items_cand
    assert (fr.restype, fr.argtypes) == L.CANDIDATES_SIGNATURES['a4r_eval_rank_cand']            # installed by lib()
    assert (ft.restype, ft.argtypes) == L.CANDIDATES_SIGNATURES['a4r_topk_items_cand']
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    # NULL mask, E = 96, misaligned operands
    assert fr(None, P(prec), P(emb), P(tgt), P(ptr), P(idx), None, P(rank), U, N1, 128) == -1
    assert fr(None, P(prec), P(emb), P(tgt), P(ptr), P(idx), P(cand), P(rank), U, N1, 96) == -1
    assert fr(None, P(prec, 4), P(emb), P(tgt), P(ptr), P(idx), P(cand), P(rank), U, N1, 64) == -1
    assert ft(None, P(prec), P(emb), P(ptr), P(idx), None, P(ids), P(sc), P(ws), U, N1, 128, 10) == -1
    for E, K in ((96, 10), (128, 0), (128, 257)):
        assert ft(None, P(prec), P(emb), P(ptr), P(idx), P(cand), P(ids), P(sc), P(ws), U, N1, E, K) == -1, (E, K)
    # the wrappers: a mask on the host, a mask of N1 - 1 bytes, a wrong dtype, K outside 1 .. 256, E = 96
    k = 10
    ids_k, sc_k = torch.full((U, k), 7, dtype=torch.int32, device=DEV), torch.full((U, k), 7.0, device=DEV)
    for bad in (cand.cpu(), cand[:-1].contiguous(), cand.int(), None):
        with pytest.raises(ValueError):
            L.eval_rank_cand(prec, emb, tgt, ptr, idx, bad, rank)
        with pytest.raises(ValueError):
            L.topk_items_cand(prec, emb, ptr, idx, bad, k, ids_k, sc_k)
    for bad_k in (0, 257):
        with pytest.raises(ValueError):
            L.topk_items_cand(prec, emb, ptr, idx, cand, bad_k, ids_k, sc_k)
    with pytest.raises(ValueError):
        L.topk_items_cand(torch.randn(U, 96, device=DEV), torch.randn(N1, 96, device=DEV), ptr, idx, cand, k, ids_k, sc_k)
    with pytest.raises(RuntimeError, match='invalid argument'):
        L.eval_rank_cand(torch.randn(U, 96, device=DEV), torch.randn(N1, 96, device=DEV), tgt, ptr, idx, cand, rank)
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all()) and bool((rank == 7).all()) and bool((ids_k == 7).all()) and bool((sc_k == 7.0).all())


def test_torch_ops_give_the_wrappers_results():
    from adapter4rec_amd import torch_ops
    ops = torch_ops.load()
    assert 'topk_rank_eval_cand' in torch_ops.OPS and 'topk_items_cand' in torch_ops.OPS
    shape = SHAPES[4]
    K, E, N1, U = shape
    d = inputs(shape)
    cand = torch.from_numpy(make_mask('half', shape, d['target'])).to(DEV)
    rank, ids, sc = run_masked(d, cand, K)
    for c in (cand, cand != 0):                                                 # uint8 and bool
        r2 = torch.zeros(U, dtype=torch.int32, device=DEV)
        ops.topk_rank_eval_cand(d['prec'], d['emb'], d['target32'], d['ptr'], d['flat'], c, r2)
        i2, s2 = ops.topk_items_cand(d['prec'], d['emb'], d['ptr'], d['flat'], c, K)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(r2.cpu().numpy(), rank)
        np.testing.assert_array_equal(i2.cpu().numpy(), ids)
        np.testing.assert_array_equal(s2.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    r2 = torch.full((U,), 7, dtype=torch.int32, device=DEV)
    for bad in (cand.cpu(), cand[:-1].contiguous(), cand.int(), cand.float(), cand[None]):      # device, shape and dtype: TORCH_CHECK
        with pytest.raises(RuntimeError, match='cand'):
            ops.topk_rank_eval_cand(d['prec'], d['emb'], d['target32'], d['ptr'], d['flat'], bad, r2)
        with pytest.raises(RuntimeError, match='cand'):
            ops.topk_items_cand(d['prec'], d['emb'], d['ptr'], d['flat'], bad, K)
    torch.cuda.synchronize()
    assert bool((r2 == 7).all())


# ------------------------------------------------------------------------------------------------------------------ API level
def test_recommend_and_eval_model_with_a_mask_on_an_id_model():
    """recommend(..., candidates=m) returns candidates only -- the unrestricted ordering with the non-candidates struck out -- and HR@10 counted
    from its lists over the users whose target is a candidate equals eval_model(..., candidates=m)."""
    from test_topk_gpu import _id_model
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import eval_model, eval_ranks, recommend
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    rng = np.random.default_rng(8)
    U = 300
    eval_seq, hist = {}, {}
    for u in range(U):
        s = list(rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False))
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    cand = rng.random(item_num + 1) < 0.5
    target = np.array([eval_seq[u][-1] for u in range(U)])
    valid = cand[target]
    assert 0 < valid.sum() < U

    class Log:
        lines = []

        def info(self, msg):
            self.lines.append(str(msg))
    hr = eval_model(model, hist, eval_seq, emb, 256, args, item_num, Log(), 'test', 0, candidates=cand)
    assert any(f'{int(valid.sum())} of {U} users' in l for l in Log.lines)
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    ids, sc = recommend(model, seqs, emb, 10, args, exclude=hist, candidates=torch.from_numpy(cand))
    ids = ids.cpu().numpy()
    assert cand[ids[ids != 0]].all()
    hits = int(sum(eval_seq[u][-1] in ids[u] for u in range(U) if valid[u]))
    assert hits == round(hr * int(valid.sum())) and abs(hits / valid.sum() - hr) < 1e-6, (hits, hr)
    assert not any(eval_seq[u][-1] in ids[u] for u in range(U) if not valid[u])
    # ranks for every listed user; a candidate target's rank is its position in the list
    ranks = eval_ranks(model, hist, eval_seq, emb, 256, args, list(range(U)), candidates=cand).cpu().numpy()
    assert ranks.shape == (U,) and (ranks >= 1).all()
    for u in np.flatnonzero(valid & (ranks <= 10)):
        assert ids[u, ranks[u] - 1] == target[u], u
    # the unrestricted ordering with the non-candidates struck out
    full, _ = recommend(model, seqs, emb, min(item_num, 256), args, exclude=hist)
    full = full.cpu().numpy()
    if item_num <= 256:
        for u in range(U):
            want = [i for i in full[u] if i != 0 and cand[i]][:10]
            assert ids[u][:len(want)].tolist() == want and (ids[u][len(want):] == 0).all(), u
    with pytest.raises(ValueError, match='one entry per table row'):
        recommend(model, seqs, emb, 10, args, exclude=hist, candidates=cand[:-1])
    with pytest.raises(ValueError, match='no candidate'):
        eval_model(model, hist, eval_seq, emb, 256, args, item_num, logging.getLogger('t'), 'test', 0, candidates=np.zeros(item_num + 1, bool))
