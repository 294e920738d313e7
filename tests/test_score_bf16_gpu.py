"""a4r_eval_rank_bf16 / a4r_topk_items_bf16 on the MI355X (include/a4r_score_bf16.h): exact ranks and lists on integer tables at every row-set, tile
and width edge, random tables against fp64 at the rounded operands, the two entries against each other, determinism across grids, the tie that
only bf16 rounding makes, argument errors, and eval_model / recommend / the text runner under score_dtype bf16 against the restatement
(tests/score_bf16_ref.py)."""
import ctypes as C
import glob
import json
import logging
import os

import numpy as np
import pytest
import torch

import score_bf16_ref as SR
from score_ce_bf16_ref import round_bf16
from topk_ref import csr, trigger_case, trigger_expected

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def cast(x):
    """fp32 array or tensor -> its bf16 copy on the device, by the library's own cast"""
    from adapter4rec_amd import _lib as L
    x = (torch.from_numpy(np.ascontiguousarray(x, np.float32)) if isinstance(x, np.ndarray) else x).to(DEV).contiguous()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=DEV)
    L.cast_bf16(x, out)
    return out


def dev_mask(cand):
    return None if cand is None else torch.from_numpy(np.ascontiguousarray(cand, np.uint8)).to(DEV)


def run_topk(prec_b, emb_b, lists, k, cand=None):
    from adapter4rec_amd import _lib as L
    ptr, flat = csr(lists)
    U = prec_b.shape[0]
    ids = torch.full((U, k), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, k), 7.0, dtype=torch.float32, device=DEV)
    L.topk_items_bf16(prec_b, emb_b, torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), k, ids, sc, dev_mask(cand))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def run_rank(prec_b, emb_b, target, lists, cand=None):
    from adapter4rec_amd import _lib as L
    ptr, flat = csr(lists)
    rank = torch.full((prec_b.shape[0],), -7, dtype=torch.int32, device=DEV)
    L.eval_rank_bf16(prec_b, emb_b, torch.from_numpy(np.asarray(target, np.int32)).to(DEV), torch.from_numpy(ptr).to(DEV),
                     torch.from_numpy(flat).to(DEV), rank, dev_mask(cand))
    torch.cuda.synchronize()
    return rank.cpu().numpy()


def make_cand(mode, rng, N1, target):
    if mode is None:
        return None
    if mode == 'all':
        return np.ones(N1, np.uint8)
    c = (rng.random(N1) < (0.1 if N1 > 100 else 0.5)).astype(np.uint8)
    c[0] = 1                                                         # the pad entry is ignored
    if mode == 'notarget':
        c[np.asarray(target)] = 0                                    # no target is a candidate: each gets the rank it would have
    return c


def valid_items(lists, U, N1, cand):
    """bool [U, N1] on the device: the items a user's rank counts / list is drawn from"""
    ok = torch.ones(U, N1, dtype=torch.bool, device=DEV)
    ok[:, 0] = False
    rows, cols = [], []
    for u, x in enumerate(lists):
        x = np.asarray(list(x)[:264], np.int64).reshape(-1)
        x = x[(x > 0) & (x < N1)]
        rows.append(np.full(x.size, u, np.int64))
        cols.append(x)
    ok[torch.from_numpy(np.concatenate(rows)).to(DEV), torch.from_numpy(np.concatenate(cols)).to(DEV)] = False
    if cand is not None:
        ok &= torch.from_numpy(np.asarray(cand) != 0).to(DEV)[None]
    return ok


def oracle_exact(prec, emb, lists, target, k, cand):
    """Integer tables: every score is an integer below 2^24, exact in bf16 operands and in fp32 sums; the fp64 product is the same number.  The
    lexsort order (score descending, id ascending) is one fp64 key: score x 2^17 - id, exact below 2^53.  -> (ids, scores, ranks)."""
    U, N1 = prec.shape[0], emb.shape[0]
    s = torch.from_numpy(prec).to(DEV).double() @ torch.from_numpy(emb).to(DEV).double().t()
    ok = valid_items(lists, U, N1, cand)
    ts = s.gather(1, torch.from_numpy(np.asarray(target, np.int64)).to(DEV)[:, None])
    ranks = 1 + ((s > ts) & ok).sum(1)
    key = torch.where(ok, s * 2.0 ** 17 - torch.arange(N1, device=DEV, dtype=torch.float64)[None], torch.full_like(s, -np.inf))
    n = min(k, N1)
    v, i = torch.topk(key, n, dim=1)
    ids = np.zeros((U, k), np.int64)
    out = np.full((U, k), -np.inf, np.float32)
    found = torch.isfinite(v)
    ids[:, :n] = torch.where(found, i, torch.zeros_like(i)).cpu().numpy()
    out[:, :n] = torch.where(found, s.gather(1, i), torch.full_like(v, -np.inf)).float().cpu().numpy()
    out[out == 0] = 0.0
    return ids, out, ranks.cpu().numpy()


# (K, E, N1, U, cand): every listed K, E, N1, U and candidate form at least once; U at every edge of 16, 32, 64 and 128 users (the workgroups of one,
# two, four and eight row sets that are instantiated) and in many workgroups; short lists where fewer than K items are left; each E with more than one item range
CASES = [
    (1, 64, 2, 1, None), (7, 128, 17, 15, 'all'), (10, 64, 14720, 16, 'sparse'), (64, 256, 65537, 17, None), (100, 512, 14720, 17, 'notarget'),
    (256, 64, 65537, 16, None), (10, 64, 65537, 4096, None), (100, 128, 14720, 4096, 'sparse'), (256, 512, 17, 16, 'all'), (7, 64, 18, 63, None),
    (256, 128, 65537, 15, 'sparse'), (64, 64, 2, 17, 'all'), (1, 256, 65, 64, 'notarget'), (10, 128, 66, 65, None), (64, 128, 65537, 33, 'sparse'),
    (10, 256, 14720, 32, None), (64, 512, 66, 31, None), (10, 512, 65537, 65, 'notarget'), (100, 64, 65, 64, None), (64, 64, 14720, 4096, 'notarget'),
    (10, 256, 14720, 4096, None), (10, 512, 14720, 1, 'sparse'), (10, 64, 14720, 129, None), (7, 128, 65537, 128, 'sparse'), (64, 64, 66, 127, None),
    (10, 128, 14720, 4096, 'notarget'),
]


@pytest.mark.parametrize('K,E,N1,U,mode', CASES)
def test_exact_on_integer_tables(K, E, N1, U, mode):
    prec, emb, lists, target = SR.integer_case(K * 7 + E + N1 + U, U, N1, E)
    cand = make_cand(mode, np.random.default_rng(K + U), N1, target)
    prec_b, emb_b = cast(prec), cast(emb)
    assert torch.equal(emb_b.float().cpu(), torch.from_numpy(emb))   # integers in [-8, 8] are bf16 numbers
    ri, rs, rr = oracle_exact(prec, emb, lists, target, K, cand)
    ids, sc = run_topk(prec_b, emb_b, lists, K, cand)
    np.testing.assert_array_equal(ids, ri)
    np.testing.assert_array_equal(sc.view(np.uint32), rs.view(np.uint32))
    np.testing.assert_array_equal(run_rank(prec_b, emb_b, target, lists, cand), rr)


@pytest.mark.parametrize('K,E', [(64, 128), (256, 64)])              # two row sets at cap = 128; one row set with four tiles in flight per wave
def test_exact_with_every_column_appended_at_every_step(K, E):
    """topk_ref.trigger_case: the append, the trigger and the compaction at the bound of 64 keys per user and step"""
    emb, prec, lists = trigger_case(E)
    prec_b, emb_b = cast(prec), cast(emb)
    assert torch.equal(emb_b.float().cpu(), torch.from_numpy(emb))   # integers up to 255 are bf16 numbers
    ri, rs = trigger_expected(emb, prec, lists, K)
    ids, sc = run_topk(prec_b, emb_b, [lists[u % 3] for u in range(prec.shape[0])], K)
    np.testing.assert_array_equal(ids, ri)
    np.testing.assert_array_equal(sc.view(np.uint32), rs.view(np.uint32))


def test_empty_and_full_lists_for_every_user():
    """every user with no list, and every user with 264 ids (repeats, pad and out-of-range ids among them), at a row-set edge"""
    U, N1, E, K = 65, 1000, 128, 10
    prec, emb, _, target = SR.integer_case(77, U, N1, E)
    rng = np.random.default_rng(78)
    full = []
    for u in range(U):
        x = rng.integers(-3, N1 + 5, size=264)
        x[:66] = x[66:132]
        x[-1] = 0
        full.append(x)
    prec_b, emb_b = cast(prec), cast(emb)
    for lists in ([np.zeros(0, np.int64)] * U, full):
        ri, rs, rr = oracle_exact(prec, emb, lists, target, K, None)
        ids, sc = run_topk(prec_b, emb_b, lists, K)
        np.testing.assert_array_equal(ids, ri)
        np.testing.assert_array_equal(sc.view(np.uint32), rs.view(np.uint32))
        np.testing.assert_array_equal(run_rank(prec_b, emb_b, target, lists), rr)


@pytest.mark.parametrize('K,E', SR.RANDOM_SHAPES)
def test_random_tables_against_fp64_at_the_rounded_operands(K, E):
    c = SR.random_case(K, E)
    U = SR.RANDOM_U
    prec_b, emb_b = cast(c['prec']), cast(c['emb'])
    np.testing.assert_array_equal(prec_b.float().cpu().numpy().view(np.uint32), round_bf16(c['prec']).view(np.uint32))      # the cast is the rule's rounding
    np.testing.assert_array_equal(emb_b.float().cpu().numpy().view(np.uint32), round_bf16(c['emb']).view(np.uint32))
    ids, sc = run_topk(prec_b, emb_b, c['lists'], K)
    s64, bound, ri, sure = c['s64'], c['bound'], c['ri'], c['sure']
    worst = 0.0
    for u in range(U):
        err = np.abs(sc[u] - s64[u, ids[u]])
        worst = max(worst, float((err / bound[u, ids[u]]).max()))
        assert np.all(err <= bound[u, ids[u]]), u                    # E x 2^-24 x sum |a b|: products exact, fp32 sums
        np.testing.assert_array_equal(ids[u][sure[u]], ri[u][:K][sure[u]])
    print(f'K = {K}, E = {E}: largest score error {worst:.3f} of its bound, {sure.mean():.3f} of the positions decided')
    assert sure.mean() >= 0.5
    rank = run_rank(prec_b, emb_b, c['target'], c['lists'])
    lo, hi = SR.rank_interval(s64, bound, c['target'], c['lists'])
    print(f'ranks: {int((lo == hi).sum())} of {U} users decided exactly, widest interval {int((hi - lo).max())}')
    assert np.all(lo <= rank) and np.all(rank <= hi), (lo, rank, hi)  # every user


@pytest.mark.parametrize('E,K,masked', [(64, 100, False), (64, 100, True), (256, 10, False), (128, 64, True), (512, 10, False)])
def test_rank_and_topk_agree_bit_for_bit(E, K, masked):
    """The bf16 form of test_topk_agrees_with_eval_rank.  The two entries hold a user in different row sets and grids ((E, K) = (64, 100): eight
    sets against one), so the agreement is also the rule's "the two rows only"."""
    rng = np.random.default_rng(3 + E + K)
    U, N1 = 1024, 65537
    emb = rng.standard_normal((N1, E)).astype(np.float32)
    tgt = rng.integers(1, N1, size=U)
    prec = emb[tgt] * 0.3 + rng.standard_normal((U, E)).astype(np.float32)      # users pointed at their targets: many rank inside the list
    cand = None
    if masked:
        cand = (rng.random(N1) < 0.3).astype(np.uint8)
        cand[tgt] = 1
    hist = []
    for u in range(U):
        h = rng.integers(1, N1, size=int(rng.integers(1, 30)))
        hist.append(h[h != tgt[u]])
    prec_b, emb_b = cast(prec), cast(emb)
    ids, sc = run_topk(prec_b, emb_b, hist, K, cand)
    rank = run_rank(prec_b, emb_b, tgt, hist, cand)
    inside = 0
    for u in range(U):
        r = int(rank[u])
        if r <= K:
            inside += 1
            assert ids[u, r - 1] == tgt[u], (u, r)
            assert int((sc[u] > sc[u, r - 1]).sum()) == r - 1, u
        else:
            assert tgt[u] not in ids[u], u
    assert inside > U // 8, inside


def test_deterministic_and_grid_independent():
    """Two calls give equal bits; a user alone (one workgroup x 32 item ranges + the merge) gets the bits it gets in the batch (many workgroups,
    few ranges), in another row of another row set.  The entries expose no range count of their own: the batch size is what moves the grid."""
    rng = np.random.default_rng(4)
    U, N1, E, K = 8192, 65537, 64, 64
    emb = rng.standard_normal((N1, E)).astype(np.float32)
    prec = rng.standard_normal((U, E)).astype(np.float32)
    lists = SR.excl_lists(rng, U, N1)
    tgt = rng.integers(1, N1, size=U)
    prec_b, emb_b = cast(prec), cast(emb)
    a, b = run_topk(prec_b, emb_b, lists, K), run_topk(prec_b, emb_b, lists, K)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    ra, rb = run_rank(prec_b, emb_b, tgt, lists), run_rank(prec_b, emb_b, tgt, lists)
    np.testing.assert_array_equal(ra, rb)
    for u in (0, 4321, U - 1):
        i1, s1 = run_topk(prec_b[u:u + 1].contiguous(), emb_b, [lists[u]], K)
        np.testing.assert_array_equal(i1[0], a[0][u])
        np.testing.assert_array_equal(s1[0].view(np.uint32), a[1][u].view(np.uint32))
        assert run_rank(prec_b[u:u + 1].contiguous(), emb_b, tgt[u:u + 1], [lists[u]])[0] == ra[u]
    sub = slice(4000, 4100)                                          # 100 users: other row sets, another range count
    i2, s2 = run_topk(prec_b[sub].contiguous(), emb_b, lists[sub], K)
    np.testing.assert_array_equal(i2, a[0][sub])
    np.testing.assert_array_equal(s2.view(np.uint32), a[1][sub].view(np.uint32))
    np.testing.assert_array_equal(run_rank(prec_b[sub].contiguous(), emb_b, tgt[sub], lists[sub]), ra[sub])


def test_not_fp32_by_another_name():
    """Two items whose fp32 scores differ but whose rounded rows are equal: the bf16 entries see a tie and give it to the smaller id, a4r_topk_items
    orders them by score, and the rank of the smaller one moves from 2 to 1."""
    from adapter4rec_amd import _lib as L
    E, N1, U = 64, 200, 3
    rng = np.random.default_rng(9)
    emb = rng.integers(-2, 3, size=(N1, E)).astype(np.float32)
    emb[3] = 4.0
    emb[5] = 4.0
    emb[5, 0] += 2.0 ** -10                                          # below bf16's resolution at 4: the rounded rows are equal
    prec = np.ones((U, E), np.float32)
    lists = [np.zeros(0, np.int64)] * U
    prec_b, emb_b = cast(prec), cast(emb)
    assert torch.equal(emb_b[3], emb_b[5])
    ids, sc = run_topk(prec_b, emb_b, lists, 2)
    assert ids.tolist() == [[3, 5]] * U and (sc == 4.0 * E).all()
    assert run_rank(prec_b, emb_b, [3] * U, lists).tolist() == [1] * U and run_rank(prec_b, emb_b, [5] * U, lists).tolist() == [1] * U
    p32, e32 = torch.from_numpy(prec).to(DEV), torch.from_numpy(emb).to(DEV)
    ptr, flat = csr(lists)
    ids32 = torch.empty(U, 2, dtype=torch.int32, device=DEV)
    sc32 = torch.empty(U, 2, dtype=torch.float32, device=DEV)
    L.topk_items(p32, e32, torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), 2, ids32, sc32)
    rank32 = torch.zeros(U, dtype=torch.int32, device=DEV)
    L.eval_rank(p32, e32, torch.full((U,), 3, dtype=torch.int32, device=DEV), torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), rank32)
    torch.cuda.synchronize()
    assert ids32.cpu().tolist() == [[5, 3]] * U and rank32.cpu().tolist() == [2] * U


def test_argument_errors_launch_nothing():
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    U, N1 = 16, 100
    emb = torch.randn(N1 + 1, 128, device=DEV).to(torch.bfloat16)
    prec = torch.randn(U, 128, device=DEV).to(torch.bfloat16)
    ptr = torch.zeros(U + 1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = torch.full((U, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, 257), 7.0, device=DEV)
    rank = torch.full((U,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    f, g = lib.a4r_topk_items_bf16, lib.a4r_eval_rank_bf16
    assert (f.restype, f.argtypes) == L.SCORE_BF16_SIGNATURES['a4r_topk_items_bf16']      # installed by lib()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for p, po, e, eo, E, K in ((prec, 0, emb, 0, 128, 0), (prec, 0, emb, 0, 128, 257), (prec, 0, emb, 0, 96, 10), (prec, 4, emb, 0, 64, 10),
                               (prec, 0, emb, 8, 64, 10)):
        assert f(None, P(p, po), P(e, eo), P(ptr), P(idx), None, P(ids), P(sc), P(ws), U, N1, E, K) == -1, (po, eo, E, K)
        if 1 <= K <= 256:
            assert g(None, P(p, po), P(e, eo), P(ptr), P(ptr), P(idx), None, P(rank), U, N1, E) == -1, (po, eo, E)
    assert f(None, P(prec), P(emb), P(ptr), P(idx), None, P(ids), P(sc), P(ws, 4), U, N1, 128, 10) == -1          # ws off 8 bytes
    assert f(None, P(prec), P(emb), P(ptr), P(idx), None, P(ids), P(sc), None, U, N1, 128, 10) == -1
    assert g(None, P(prec), P(emb), P(ptr), P(ptr), P(idx), None, None, U, N1, 128) == -1
    assert g(None, P(prec), P(emb), P(ptr), P(ptr), P(idx), None, P(rank), 0, N1, 128) == -1 and g(None, P(prec), P(emb), P(ptr), P(ptr), P(idx), None, P(rank), U, 1, 128) == -1
    assert L.topk_bf16_ws_bytes(U, N1, 128, 0) == 0 and L.topk_bf16_ws_bytes(U, N1, 128, 257) == 0 and L.topk_bf16_ws_bytes(U, N1, 96, 10) == 0
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all()) and bool((rank == 7).all())


# ------------------------------------------------------------------------------------------------------------------ API and runner level
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _id_model():
    import test_id_tower_cpu as CPU
    model, fx, _ = CPU.build('sasrec', compute_dtype='fp32')
    args = CPU.make_args(arch='sasrec', adapter_type='None')
    return model.to(DEV), args, int(fx['item_num'])


def _record(monkeypatch):
    """The real wrappers, recording what they are handed: the fp32 sources of every cast, and the operands and lists of every bf16 entry call."""
    from adapter4rec_amd import _lib as L
    seen = dict(cast=[], rank=[], topk=[])
    real = {n: getattr(L, n) for n in ('cast_bf16', 'eval_rank_bf16', 'topk_items_bf16')}

    def cast_bf16(src, dst, n=None):
        real['cast_bf16'](src, dst, n)
        seen['cast'].append((src.detach().clone(), dst))

    def eval_rank_bf16(*a):
        seen['rank'].append([x.detach().clone() if isinstance(x, torch.Tensor) else x for x in a])
        return real['eval_rank_bf16'](*a)

    def topk_items_bf16(*a):
        seen['topk'].append([x.detach().clone() if isinstance(x, torch.Tensor) else x for x in a])
        return real['topk_items_bf16'](*a)
    for n, fn in (('cast_bf16', cast_bf16), ('eval_rank_bf16', eval_rank_bf16), ('topk_items_bf16', topk_items_bf16)):
        monkeypatch.setattr(L, n, fn, raising=False)
    for n in ('eval_rank', 'eval_rank_cand', 'topk_items', 'topk_items_cand'):
        monkeypatch.setattr(L, n, lambda *a, **k: pytest.fail('an fp32 entry under score_dtype bf16'), raising=False)
    return seen


def _users(item_num, args, U, seed):
    rng = np.random.default_rng(seed)
    eval_seq, hist = {}, {}
    for u in range(U):
        s = [int(x) for x in rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False)]
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    return eval_seq, hist


def test_eval_model_and_recommend_bf16_on_the_id_tower(monkeypatch):
    """eval_model(score_dtype='bf16'): HR@10 / nDCG@10 equal to the restatement's at the rounded operands (the user vectors the cast was handed,
    the table, fp64 scores); HR@10 computed from recommend(score_dtype='bf16') equals eval_model's."""
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    U = 300
    eval_seq, hist = _users(item_num, args, U, 7)
    seen = _record(monkeypatch)
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 256, args, item_num, log, 'test', 0, score_dtype='bf16')
    torch.cuda.synchronize()
    assert len(seen['cast']) == 1 + len(seen['rank']) and torch.equal(seen['cast'][0][0], emb.float())      # the table once, each batch's vectors once
    emb_np = emb.float().cpu().numpy()
    for src, dst in seen['cast']:                                    # the cast is the rule's rounding
        np.testing.assert_array_equal(dst.float().cpu().numpy().view(np.uint32), round_bf16(src.cpu().numpy()).view(np.uint32))
    prec = torch.cat([c[0] for c in seen['cast'][1:]]).cpu().numpy()
    assert prec.shape == (U, emb.shape[1])
    target = np.array([eval_seq[u][-1] for u in range(U)])
    hlists = [hist[u].numpy() for u in range(U)]
    s64, bound = SR.scores64(prec, emb_np), SR.sum_bound(prec, emb_np)
    want = SR.rank_reference(s64, target, hlists)
    lo, hi = SR.rank_interval(s64, bound, target, hlists)
    print(f'{int((lo == hi).sum())} of {U} ranks decided by fp64 beyond the summation bound')
    hit, ndcg = SR.hit_ndcg(want)
    line = [l for l in log.lines if 'test_results' in l][0]
    got = [float(x) for x in line.split()[1:]]
    print(f'HR@10 {hr:.6f} nDCG@10 {got[1] / 100:.6f}; the restatement {hit:.6f} {ndcg:.6f}')
    assert abs(hr - hit) < 1e-6 and abs(got[1] / 100 - ndcg) < 1e-6
    ids, sc = recommend(model, {u: eval_seq[u][:-1] for u in range(U)}, emb, 10, args, exclude=hist, score_dtype='bf16')
    ids = ids.cpu().numpy()
    hits = int(sum(eval_seq[u][-1] in ids[u] for u in range(U)))
    assert hits == round(hr * U) and abs(hits / U - hr) < 1e-6, (hits, hr)
    assert len(seen['topk']) == 1 and seen['topk'][0][0].dtype == torch.bfloat16 and seen['topk'][0][1].dtype == torch.bfloat16
    # the fp32 path on the same model, for the record (logged, not asserted)
    monkeypatch.undo()
    log32 = _Log()
    hr32 = eval_model(model, hist, eval_seq, emb, 256, args, item_num, log32, 'test', 0)
    ids32, _ = recommend(model, {u: eval_seq[u][:-1] for u in range(U)}, emb, 10, args, exclude=hist)
    same = float((ids32.cpu().numpy() == ids).all(1).mean())
    print(f'fp32 on the same model: {[l for l in log32.lines if "test_results" in l][0]}; bf16: {line}; identical top-10 lists {same:.3f}')
    assert 0.0 <= hr32 <= 1.0


def test_text_runner_recommend_bf16_writes_the_restatements_file(tmp_path, monkeypatch):
    """train one epoch through run.py, then one run of --mode recommend --score_dtype bf16 from its checkpoint: every line of the file is the
    restatement's list at the operands the run rounded (fp64 scores of the recorded bf16 operands, the seen sequence excluded), up to the gap
    rule; the cast it used is the rule's rounding of the fp32 vectors it was handed; the log names the dtype."""
    import test_text_run as TR
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    root = str(tmp_path)
    data = TR.write_toy(root)
    cp = os.path.join(root, 'pretrained_models', 'bert', 'bert_tiny', 'config.json')
    c = json.load(open(cp))
    c.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    json.dump(c, open(cp, 'w'))
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data, '--dataset', 'toy', '--behaviors', 'behaviors.tsv', '--news', 'news.tsv', '--bert_model_load', 'bert_tiny',
              '--freeze_paras_before', '0', '--adapter_type', 'houslby', '--adding_adapter_to', 'all', '--fine_tune_to', 'None',
              '--pretrained_model_name', 'None', '--embedding_dim', '64', '--batch_size', '16', '--num_workers', '1', '--logging_num', '3',
              '--testing_num', '1', '--max_seq_len', '20', '--min_seq_len', '5', '--lr', '1e-3', '--adapter_bert_lr', '1e-3',
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'sbf']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    seen = _record(monkeypatch)
    logged = []

    class Keep(logging.Handler):
        def emit(self, record):
            logged.append(record.getMessage())
    logging.getLogger('Log_file').addHandler(Keep())                  # (TR._run removes the run's handlers when it ends)
    out = os.path.join(root, 'rec.tsv')
    k = 7
    TR._run(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', str(k), '--recommend_out', out, '--score_dtype', 'bf16'],
            monkeypatch, dict(loss=[], batch=[], eval=[]))
    assert any(l.startswith('score dtype: bf16') for l in logged), logged
    for src, dst in seen['cast']:
        np.testing.assert_array_equal(dst.float().cpu().numpy().view(np.uint32), round_bf16(src.cpu().numpy()).view(np.uint32))
    assert len(seen['topk']) >= 1 and len(seen['cast']) == 1 + len(seen['topk'])
    lines = [l.rstrip('\n').split('\t') for l in open(out)]
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    user_names, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    assert [l[0] for l in lines] == list(user_names)
    u = 0
    for call in seen['topk']:
        prec_b, emb_b, ptr, flat, kk = call[:5]
        assert prec_b.dtype == torch.bfloat16 and emb_b.dtype == torch.bfloat16 and kk == k and call[7] is None
        p, t = prec_b.double().cpu().numpy(), emb_b.double().cpu().numpy()
        s64 = p @ t.T
        bound = p.shape[1] * 2.0 ** -24 * (np.abs(p) @ np.abs(t).T)
        pp, ff = ptr.cpu().numpy().astype(np.int64), flat.cpu().numpy().astype(np.int64)
        excl = [ff[pp[j]:pp[j + 1]] for j in range(p.shape[0])]
        ri, rs = SR.topk_reference_cand(s64, excl, k + 1)
        for j in range(p.shape[0]):
            if u >= len(lines):                                      # (the sampler's tail repeats the last users)
                break
            items, scores = lines[u][1].split(' '), np.array([float(x) for x in lines[u][2].split(' ')])
            assert len(items) == len(scores) == k
            sep = np.concatenate([[True], -np.diff(rs[j]) > bound[j].max()])
            sure = sep[:k] & sep[1:k + 1]
            want = [item_names[i] for i in ri[j][:k]]
            assert [x for x, s in zip(items, sure) if s] == [x for x, s in zip(want, sure) if s], lines[u][0]
            assert sure.mean() >= 0.5, lines[u][0]
            got_ids = [item_names.index(x) for x in items]
            assert np.all(np.abs(scores - s64[j, got_ids]) <= bound[j, got_ids] + 1e-6 * np.abs(scores)), lines[u][0]      # (%.9g in the file)
            assert not set(got_ids) & set(excl[j].tolist())
            u += 1
    assert u == len(lines) > 0
