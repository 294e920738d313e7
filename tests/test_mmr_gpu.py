"""a4r_mmr_rerank on the MI355X (include/a4r_diversify.h), against the fp64 restatement of tests/mmr_ref.py.

Exact cases: table rows of exactly 64 non-zero entries +-2^k (norms 8 * 2^k, every dot product and cosine a multiple of 1/64 and exact in fp32),
integer pool scores whose range is a power of two (relevance k / 2^q) and lambda in {0, 0.25, 0.5, 1}: every v is exact in fp32, ties are exact
ties, so ids and score bits are compared exactly and ILD to 1e-6 relative.  Random case: a Gaussian table, decided by the margin rule
(mmr_ref.tau).  End to end: recommend(diversify=) on the device against the restatement applied to the device's own pool."""
import numpy as np
import pytest
import torch

import mmr_ref as MR
from topk_ref import csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_mmr(emb, pid, ps, lam, K, want_ild=True):
    """emb: a device tensor; pid, ps: numpy -> (ids, scores, ild or None) as numpy"""
    from adapter4rec_amd import _lib as L
    U = pid.shape[0]
    ids = torch.full((U, K), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, K), 7.0, dtype=torch.float32, device=DEV)
    ild = torch.full((U,), -7.0, dtype=torch.float32, device=DEV) if want_ild else None
    L.mmr_rerank(emb, dev(pid), dev(ps), lam, K, ids, sc, ild)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), (ild.cpu().numpy() if want_ild else None)


def assert_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def assert_exact(emb_np, emb, pid, ps, lam, K, what):
    gi, gs, gd = run_mmr(emb, pid, ps, lam, K)
    ri, rs, rd, _, _ = MR.mmr_reference(emb_np, pid, ps, lam, K)
    np.testing.assert_array_equal(gi, ri, err_msg=str(what))
    assert_bits(gs, rs)
    np.testing.assert_allclose(gd, rd, rtol=1e-6, atol=1e-12, err_msg=str(what))
    return gi, gs, gd


# ------------------------------------------------------------------ 1: exact cases
POOL_SIZES = (1, 2, 15, 16, 17, 100, 255, 256)


@pytest.mark.parametrize('E', (64, 128, 256, 512))
def test_exact_cases_at_every_pool_size(E):
    """U in {1, 3} x P on either side of the 16 rows a pass takes and of the 256 threads x K in {1, 10, P} x the four lambdas on a 300-row table,
    the pools with pads at the tail and in the middle, ids that are negative or >= N1, NaN / +-inf scores, a repeated id, the twins and the
    zero-norm row (mmr_ref.exact_pool); and the same pool sizes on the two-row table, where every valid entry is item 1."""
    cases = 0
    for N1 in (300, 2):
        emb_np = MR.exact_table(N1, E)
        emb = dev(emb_np)
        for U in (1, 3):
            for P in POOL_SIZES:
                pid, ps = MR.exact_pool(U, P, N1, seed=10 * P + U)
                for K in sorted({1, min(10, P), P}):
                    for lam in (MR.LAMBDAS if N1 == 300 else (0.5,)):
                        gi, _, _ = assert_exact(emb_np, emb, pid, ps, lam, K, (E, N1, U, P, K, lam))
                        assert ((gi >= 0) & (gi < N1)).all()
                        cases += 1
    assert cases == 2 * (1 + 2 + 6 * 3) * (4 + 1)                                 # two U x 21 (P, K) pairs x (four lambdas at N1 = 300 + one at N1 = 2)


def test_exact_special_pools():
    """the twin of pick 1 is not pick 2 at lambda = 0.5 (and is at lambda = 1); an all-equal-score pool; the zero-norm row; a repeated id; fewer
    valid entries than K; nothing valid at all"""
    E, N1 = 64, 300
    emb_np = MR.exact_table(N1, E)
    emb = dev(emb_np)
    a, b = MR.TWINS
    z, other = MR.ZERO_ROW, 20
    i32, f32 = (lambda x: np.asarray(x, np.int32)), (lambda x: np.asarray(x, np.float32))
    pid, ps = i32([[a, b, other, z]]), f32([[8, 7, 4, 0]])
    gi, gs, _ = assert_exact(emb_np, emb, pid, ps, 0.5, 4, 'twins')
    assert gi[0, 0] == a and gi[0, 1] != b and sorted(gi[0].tolist()) == sorted([a, b, other, z])
    gi, _, _ = assert_exact(emb_np, emb, pid, ps, 1.0, 4, 'twins, lambda 1')
    assert gi[0].tolist() == [a, b, other, z]
    gi, _, _ = assert_exact(emb_np, emb, i32([[a, b, z]]), f32([[3, 2, 1]]), 0.0, 3, 'zero norm')
    assert gi[0].tolist() == [a, z, b]
    gi, gs, gd = assert_exact(emb_np, emb, i32([[a, a]]), f32([[2, 1]]), 0.5, 2, 'repeated id')
    assert gi[0].tolist() == [a, a] and gs[0].tolist() == [2.0, 1.0] and gd[0] == 0.0
    rng = np.random.default_rng(5)
    pid = rng.integers(1, N1, size=(3, 40)).astype(np.int32)
    for lam in MR.LAMBDAS:
        assert_exact(emb_np, emb, pid, np.full((3, 40), 5.0, np.float32), lam, 10, ('all equal', lam))          # range 0: r = 1 everywhere
    gi, gs, gd = assert_exact(emb_np, emb, i32([[other, 0, a, 999, -1, b]]), f32([[5, -np.inf, 5, 5, 5, np.nan]]), 0.25, 6, 'fewer than K')
    assert gi[0].tolist() == [other, a, 0, 0, 0, 0] and np.isneginf(gs[0, 2:]).all()
    gi, gs, gd = assert_exact(emb_np, emb, i32([[0, -1, N1, a]]), f32([[1, 1, 1, np.inf]]), 0.5, 3, 'nothing valid')
    assert (gi == 0).all() and np.isneginf(gs).all() and gd[0] == 0.0


def test_lambda_one_on_topk_items_output_is_topk_items():
    """a4r_topk_items' pool of 100 / 256 under lambda = 1 is a4r_topk_items at K, bit for bit -- ids, scores and the pad slots of a user whose
    exclusion list leaves fewer items than the pool holds"""
    from adapter4rec_amd import _lib as L
    E, N1, U = 128, 300, 5
    rng = np.random.default_rng(6)
    emb = dev(MR.exact_table(N1, E))
    prec = dev(rng.integers(-2, 3, size=(U, E)).astype(np.float32))
    excl = [rng.permutation(N1 - 1)[:n] + 1 for n in (0, 10, 60, 200, 264)]
    xp, xf = csr(excl)
    xp, xf = dev(xp), dev(xf)

    def topk(K):
        ids = torch.empty(U, K, dtype=torch.int32, device=DEV)
        sc = torch.empty(U, K, dtype=torch.float32, device=DEV)
        L.topk_items(prec, emb, xp, xf, K, ids, sc)
        return ids, sc
    for P in (100, 256):
        pool_i, pool_s = topk(P)
        assert P < 256 or bool((pool_i == 0).any())
        for K in (1, 10, P):
            want_i, want_s = topk(K)
            ids = torch.full((U, K), -7, dtype=torch.int32, device=DEV)
            sc = torch.full((U, K), 7.0, dtype=torch.float32, device=DEV)
            L.mmr_rerank(emb, pool_i, pool_s, 1.0, K, ids, sc)
            torch.cuda.synchronize()
            assert torch.equal(ids, want_i), (P, K)
            assert_bits(sc.cpu().numpy(), want_s.cpu().numpy())


def test_no_ild_a_second_stream_and_a_second_call_give_the_same_bits():
    E, N1, U, P, K = 256, 300, 3, 100, 10
    emb_np = MR.exact_table(N1, E)
    emb = dev(emb_np)
    pid, ps = MR.exact_pool(U, P, N1, seed=77)
    base = run_mmr(emb, pid, ps, 0.5, K)
    ri, rs, rd, _, _ = MR.mmr_reference(emb_np, pid, ps, 0.5, K)
    np.testing.assert_array_equal(base[0], ri)
    again = run_mmr(emb, pid, ps, 0.5, K)
    none = run_mmr(emb, pid, ps, 0.5, K, want_ild=False)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = run_mmr(emb, pid, ps, 0.5, K)
    s.synchronize()
    for got in (again, other):
        np.testing.assert_array_equal(got[0], base[0])
        assert_bits(got[1], base[1])
        assert_bits(got[2], base[2])
    assert none[2] is None
    np.testing.assert_array_equal(none[0], base[0])
    assert_bits(none[1], base[1])


def test_more_users_than_the_grid_holds():
    """65 536 workgroups stride over the users: the users behind them get their own lists"""
    E, N1, U, P, K = 64, 300, 65536 + 3, 3, 2
    emb_np = MR.exact_table(N1, E)
    rng = np.random.default_rng(8)
    pid = rng.integers(0, N1 + 1, size=(U, P)).astype(np.int32)
    ps = rng.integers(0, 5, size=(U, P)).astype(np.float32) * 2.0
    ps[:, 0], ps[:, 1] = 8.0, 0.0                                                 # a range of 8 wherever entries 0 and 1 are valid
    gi, gs, gd = run_mmr(dev(emb_np), pid, ps, 0.5, K)
    both = np.flatnonzero((pid[:, 0] >= 1) & (pid[:, 0] < N1) & (pid[:, 1] >= 1) & (pid[:, 1] < N1))
    pick = np.concatenate([both[:40], both[-40:], np.arange(U - 3, U)])
    assert (both >= 65536).any()
    ri, rs, rd, _, _ = MR.mmr_reference(emb_np, pid[pick], ps[pick], 0.5, K)
    keep = np.isin(pick, both)                                                    # (the three last users may have another range: ids only)
    np.testing.assert_array_equal(gi[pick][keep], ri[keep])
    assert_bits(gs[pick][keep], rs[keep])
    np.testing.assert_allclose(gd[pick][keep], rd[keep], rtol=1e-6, atol=1e-12)
    assert ((gi >= 0) & (gi < N1)).all() and (gi[:, 0] != 0).mean() > 0.9


# ------------------------------------------------------------------ 2: the random case, decided by the margin rule
@pytest.mark.parametrize('E', (64, 512))
def test_random_case_against_fp64(E):
    """Gaussian table, uniform scores, U = 64, P = 100, K = 10, lambda = 0.7: the kernel's list equals the restatement's for every user whose
    smallest margin exceeds tau = 4 (E + 16) 2^-24, and up to the first round under tau for the others -- at most 10 % of the users, asserted on
    the restatement before the kernel's output is looked at."""
    emb_np, pid, ps = MR.gaussian_case(E)
    ri, rs, rd, margin, margins = MR.mmr_reference(emb_np, pid, ps, 0.7, 10)
    tau = MR.tau(E)
    under = margin <= tau
    print(f'E = {E}: tau = {tau:.3g}, {int(under.sum())} of 64 users under it, smallest margin {margin.min():.3g}')
    assert under.mean() <= 0.10
    gi, gs, gd = run_mmr(dev(emb_np), pid, ps, 0.7, 10)
    np.testing.assert_array_equal(gi[~under], ri[~under])
    assert_bits(gs[~under], rs[~under])
    np.testing.assert_allclose(gd[~under], rd[~under], rtol=0, atol=2 * tau)     # a mean of 1 - c, every c within the dot's bound
    for u in np.flatnonzero(under):
        first = int(np.argmax(margins[u] <= tau))
        np.testing.assert_array_equal(gi[u, :first], ri[u, :first])
    assert int((gi != ri).any(1).sum()) <= int(under.sum())
    print(f'E = {E}: {int((gi != ri).any(1).sum())} users differ from the restatement')


# ------------------------------------------------------------------ 3: end to end
@pytest.mark.parametrize('mode', ('full', 'candidates', 'candidate_lists'))
def test_recommend_diversified_on_the_device(monkeypatch, mode):
    """recommend(diversify=) on the small ID model with an exact table: the lists are the restatement's re-ranking of the pool the device's own
    top-K entry of the mode produced"""
    from test_topk_gpu import _id_model
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend
    model, args, item_num = _id_model()
    E = int(args.embedding_dim)
    emb_np = MR.exact_table(item_num + 1, E, seed=3)
    emb = dev(emb_np)
    rng = np.random.default_rng(12)
    U, k, pool, lam = 40, 10, 32, 0.5
    seqs = {u: [int(x) for x in rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 1)), replace=False)] for u in range(U)}
    kw = {}
    if mode == 'candidates':
        mask = rng.random(item_num + 1) < 0.6
        mask[list(MR.TWINS)] = True
        kw = dict(candidates=mask)
    elif mode == 'candidate_lists':
        kw = dict(candidate_lists={u: rng.integers(0, item_num + 2, size=int(rng.integers(0, 90))) for u in range(U) if u % 5 != 4})
    used = dict(full='topk_items', candidates='topk_items_cand', candidate_lists='topk_lists')[mode]
    at = dict(full=(5, 6), candidates=(6, 7), candidate_lists=(8, 9))[mode]
    pools = []
    real = getattr(L, used)

    def recording(*a):
        out = real(*a)
        pools.append((a[at[0]].clone(), a[at[1]].clone()))
        return out
    monkeypatch.setattr(L, used, recording, raising=False)
    for name in ('topk_items', 'topk_items_cand', 'topk_lists'):
        if name != used:
            monkeypatch.setattr(L, name, lambda *a, **k: pytest.fail('a top-K entry of another mode'), raising=False)
    ids, sc = recommend(model, seqs, emb, k, args, diversify=Diversify(lam, pool), **kw)
    torch.cuda.synchronize()
    assert len(pools) == 1 and tuple(pools[0][0].shape) == (U, pool)
    pool_i, pool_s = pools[0][0].cpu().numpy(), pools[0][1].cpu().numpy()
    ri, rs, _, margin, _ = MR.mmr_reference(emb_np, pool_i, pool_s, lam, k)
    print(f'{mode}: smallest margin that is no tie {margin[margin > 0].min():.3g}')
    np.testing.assert_array_equal(ids.cpu().numpy(), ri)
    assert_bits(sc.cpu().numpy(), rs)
    assert (ri != pool_i[:, :k]).any() and ids.dtype == torch.long
    plain, _ = recommend(model, seqs, emb, k, args, **kw)
    np.testing.assert_array_equal(plain.cpu().numpy(), pool_i[:, :k])             # without diversify: the pool's head
