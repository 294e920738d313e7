"""a4r_eval_draw_negatives / a4r_eval_rank_sampled on the MI355X (include/a4r_eval_negatives.h): the draws bit for bit against the restatement
of tests/eval_neg_ref.py at the edges of N, of the history, of the target, of m and of the weights; the fused rank equal to a4r_eval_rank_lists on
the materialised draws; ranks inside the fp64 bounds; exact ranks on integer tables with ties and forced duplicates; and eval_model with
--eval_negatives on a tiny ID model, replayed through the written file and --candidate_lists."""
import numpy as np
import pytest
import torch

import eval_neg_ref as NR
import lists_ref as LR
from topk_ref import csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 0x5EEDCAFEF00D1234
SAMPLINGS = ('uniform', 'pop')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_cdf(cdf):
    return None if cdf is None else dev(np.asarray(cdf, np.int64))


def run_draw(hists, target, keys, N1, n, seed, cdf):
    """-> (ids [U, n], err) from a4r_eval_draw_negatives"""
    from adapter4rec_amd import _lib as L
    U = len(target)
    hp, hf = csr(hists)
    out = torch.full((U, n), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.eval_draw_negatives(dev(hp), dev(hf), dev(np.asarray(target, np.int32)), dev(np.asarray(keys, np.int32)), dev_cdf(cdf), seed, N1, out, err)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(err.item())


def run_sampled(p, e, hists, target, keys, n, seed, cdf):
    """-> (rank [U], err) from a4r_eval_rank_sampled"""
    from adapter4rec_amd import _lib as L
    U = len(target)
    hp, hf = csr(hists)
    rank = torch.full((U,), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.eval_rank_sampled(p, e, dev(np.asarray(target, np.int32)), dev(hp), dev(hf), dev(np.asarray(keys, np.int32)), dev_cdf(cdf), seed, n, rank, err)
    torch.cuda.synchronize()
    return rank.cpu().numpy(), int(err.item())


def run_lists_on(p, e, hists, target, ids):
    """a4r_eval_rank_lists on materialised draws ids [U, n]"""
    from adapter4rec_amd import _lib as L
    U, n = ids.shape
    hp, hf = csr(hists)
    rank = torch.full((U,), -7, dtype=torch.int32, device=DEV)
    ptr = (n * np.arange(U + 1)).astype(np.int32)
    L.eval_rank_lists(p, e, dev(np.asarray(target, np.int32)), dev(ptr), dev(ids.astype(np.int32).reshape(-1)), n, dev(hp), dev(hf), rank)
    torch.cuda.synchronize()
    return rank.cpu().numpy()


def pop_counts(rng, N1, big=True):
    """occurrence counts with zero-count items and, ``big``, counts of 2^40 (the 64-bit path)"""
    cnt = rng.integers(0, 40, size=N1 - 1).astype(object)
    cnt[rng.random(N1 - 1) < 0.3] = 0
    if big:
        for i in rng.choice(N1 - 1, size=max(2, (N1 - 1) // 50), replace=False):
            cnt[i] = 2 ** 40 + int(rng.integers(0, 5))
    return [int(c) for c in cnt]


# ------------------------------------------------------------------ 1: the draws, bit for bit
def edge_users(N1, rng, cnt):
    """histories that are empty, of 1 id, of 264 ids with repeats, zeros, negative and >= N1 ids, longer than 264 (the rest is not read); targets
    inside and outside the history and targets that are no item; where N1 is small, users whose D leaves one candidate (m = 1) and none (m = 0),
    under uniform sampling and, ``cnt`` given, under the weights; user keys 0 and 2^31 - 1"""
    hists, target = [], []
    add = lambda h, t: (hists.append(np.asarray(h, np.int64)), target.append(int(t)))
    add([], 5)
    add([], 0)                                                                    # a target that is no item
    add([7], 7)                                                                   # the target inside the history
    add([7], 8)
    add([3], N1 + 4)
    add([N1 - 1], -2)
    for k in range(4):
        h = rng.integers(-3, N1 + 5, size=264)
        h[:66] = h[66:132]                                                        # repeats
        h[-1] = 0
        add(h, (h[5], int(rng.integers(1, N1)), 0, N1)[k])
    add(rng.integers(1, N1, size=300), 1)                                         # only the first 264 ids count
    for _ in range(5):
        add(rng.integers(1, N1, size=int(rng.integers(2, 60))), int(rng.integers(1, N1)))
    if N1 - 1 <= 264:
        everything = np.arange(1, N1)
        a = int(rng.integers(1, N1))
        add(everything, a)                                                        # uniform: m = 0
        add(everything[everything != a], a)                                       # m = 0: the target is the one item left
        b = 1 + a % (N1 - 1)
        add(everything[everything != a], b)                                       # m = 1: every draw is a
        add(np.concatenate([everything[everything != a], [0, -1, N1, b, b]]), 0)  # m = 1, the target no item
        if cnt is not None:
            pos = [i + 1 for i, c in enumerate(cnt) if c > 0]
            one = [i + 1 for i, c in enumerate(cnt) if c == 1]
            assert one
            add(pos, 0)                                                           # weighted: m = 0 although zero-count items are left
            add([i for i in pos if i != one[0]], 0)                               # m = 1: every draw is one[0]
    keys = rng.integers(-2 ** 31, 2 ** 31, size=len(target))
    keys[0], keys[1], keys[2] = 0, 2 ** 31 - 1, 0                                  # (a key may repeat: the draws then differ through D alone)
    return hists, target, keys


_DRAW_CASES = {}


def draw_case(N1, sampling):
    key = (N1, sampling)
    if key not in _DRAW_CASES:
        rng = np.random.default_rng(700 + N1)
        cnt = pop_counts(rng, N1)
        if N1 <= 265:
            cnt[11] = 1
        cdf = NR.make_cdf(cnt, N1) if sampling == 'pop' else None
        hists, target, keys = edge_users(N1, rng, cnt if sampling == 'pop' else None)
        _DRAW_CASES[key] = (hists, target, keys, cdf)
    return _DRAW_CASES[key]


@pytest.mark.parametrize('sampling', SAMPLINGS)
@pytest.mark.parametrize('n', [1, 63, 64, 65, 100, 257, 4096])
@pytest.mark.parametrize('N1', [200, 50021])
def test_draws_equal_the_restatement_bit_for_bit(N1, n, sampling):
    hists, target, keys, cdf = draw_case(N1, sampling)
    want, want_err = NR.draw_negatives(hists, target, keys, N1, n, SEED, cdf)
    got, err = run_draw(hists, target, keys, N1, n, SEED, cdf)
    np.testing.assert_array_equal(got, want)
    assert err == want_err
    ms = [NR.user_draws(h, t, k, N1, 1, SEED, cdf)[1] for h, t, k in zip(hists, target, keys)]
    if N1 == 200:
        assert want_err == sum(m < 1 for m in ms) >= 2 and ms.count(1) >= (1 if sampling == 'pop' else 2)      # m = 0 users are counted, m = 1 users draw their one candidate
        for u in np.flatnonzero(np.array(ms) == 1):
            assert len(set(got[u].tolist())) == 1 and got[u, 0] > 0
        assert all((got[u] == 0).all() for u in range(len(ms)) if ms[u] < 1)
    else:
        assert want_err == 0 and (got > 0).all()
    if sampling == 'pop':
        assert max(ms) > 2 ** 40                                                  # the 64-bit path
        cnt = np.diff(np.asarray(cdf, dtype=object))
        assert all(cnt[i - 1] > 0 for i in np.unique(got[got > 0]))             # no zero-count item
    for u in range(len(ms)):                                                      # never a member of D
        assert not set(got[u].tolist()) & set(NR.exclusion_set(hists[u], target[u], N1)), u


def test_draws_do_not_depend_on_the_batch():
    """a user's draws are a function of (seed, key, D, weights): the same in a batch of one, in another order, beside other users"""
    N1 = 50021
    hists, target, keys, cdf = draw_case(N1, 'pop')
    full, _ = run_draw(hists, target, keys, N1, 100, SEED, cdf)
    perm = np.random.default_rng(3).permutation(len(target))
    got, _ = run_draw([hists[i] for i in perm], [target[i] for i in perm], keys[perm], N1, 100, SEED, cdf)
    np.testing.assert_array_equal(got, full[perm])
    one, _ = run_draw(hists[9:10], target[9:10], keys[9:10], N1, 100, SEED, cdf)
    np.testing.assert_array_equal(one, full[9:10])
    other, _ = run_draw(hists, target, keys, N1, 100, SEED + 1, cdf)
    assert (other != full).mean() > 0.9                                           # another seed: other draws


# ------------------------------------------------------------------ 2: the fused rank is the list kernel on the materialised draws
_RANDOM = {}


def random_tables(E):
    """lists_ref.random_case's tables, exclusion lists (here: the histories) and targets, on the device once per E; user keys of their own"""
    if E not in _RANDOM:
        prec, emb, _, excl, target = LR.random_case(E)
        keys = np.random.default_rng(5).integers(0, 2 ** 31, size=len(target))
        rng = np.random.default_rng(6)
        cdf = NR.make_cdf(pop_counts(rng, emb.shape[0], big=False), emb.shape[0])
        _RANDOM[E] = (prec, emb, excl, target, keys, cdf, dev(prec), dev(emb))
    return _RANDOM[E]


@pytest.mark.parametrize('sampling', SAMPLINGS)
@pytest.mark.parametrize('n', [1, 100, 1000, 4096])
@pytest.mark.parametrize('E', [64, 128, 256, 512])
def test_fused_rank_equals_the_list_kernel_on_the_draws(E, n, sampling):
    prec, emb, hists, target, keys, cdf, p, e = random_tables(E)
    cdf = cdf if sampling == 'pop' else None
    N1 = emb.shape[0]
    ids, err = run_draw(hists, target, keys, N1, n, SEED, cdf)
    assert err == 0 and (ids > 0).all() and (ids < N1).all()
    want = run_lists_on(p, e, hists, target, ids)
    got, err2 = run_sampled(p, e, hists, target, keys, n, SEED, cdf)
    np.testing.assert_array_equal(got, want)
    assert err2 == 0 and (n == 1 or (got > 1).any())


def test_fused_rank_with_more_users_than_the_grid_holds():
    U, E, n, N1 = 65537, 64, 1, 64
    rng = np.random.default_rng(77)
    emb = rng.standard_normal((N1, E)).astype(np.float32)
    prec = rng.standard_normal((U, E)).astype(np.float32)
    target = rng.integers(0, N1, size=U)                                          # (0: no item, rank 1)
    hist_len = rng.integers(0, 4, size=U)
    flat = rng.integers(0, N1 + 1, size=int(hist_len.sum()) + 1).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(hist_len)]).astype(np.int32)
    hists = [flat[ptr[u]:ptr[u + 1]] for u in range(U)]
    keys = np.arange(U, dtype=np.int64) * 32749 % (2 ** 31)
    p, e = dev(prec), dev(emb)
    ids, err = run_draw(hists, target, keys, N1, n, SEED, None)
    for u in (0, 1, 4242, 65535, 65536):                                          # users on both sides of the stride against the restatement
        np.testing.assert_array_equal(ids[u], NR.user_draws(hists[u], target[u], keys[u], N1, n, SEED)[0])
    want = run_lists_on(p, e, hists, target, ids)
    got, err2 = run_sampled(p, e, hists, target, keys, n, SEED, None)
    np.testing.assert_array_equal(got, want)
    assert err == err2 == 0 and set(np.unique(got).tolist()) == {1, 2} and (got[target == 0] == 1).all()


# ------------------------------------------------------------------ 3: ranks inside the fp64 bounds
@pytest.mark.parametrize('E,n', [(64, 1000), (128, 1000), (256, 200), (512, 200)])
def test_ranks_inside_the_fp64_bounds(E, n):
    """lo[u] <= rank[u] <= hi[u]: lo counts the distinct draws with s64 > t64 + b, hi those with s64 > t64 - b, b = the sum of the two pairs' fp32
    summation bounds E * 2^-24 * sum |a b| (lists_ref.fp64_reference's).  At most a quarter of the users may have lo != hi -- a condition on the
    test, which would otherwise decide nothing: with independent uniform draws the reference alone leaves 1, 4, 0 and 5 of 48 users undecided."""
    prec, emb, hists, target, keys, _, p, e = random_tables(E)
    N1 = emb.shape[0]
    got, err = run_sampled(p, e, hists, target, keys, n, SEED, None)
    ids, _ = NR.draw_negatives(hists, target, keys, N1, n, SEED)
    p64, e64 = prec.astype(np.float64), emb.astype(np.float64)
    s64 = p64 @ e64.T
    bound = E * 2.0 ** -24 * (np.abs(p64) @ np.abs(e64).T)
    undecided = 0
    for u in range(prec.shape[0]):
        d = np.unique(ids[u])
        b = bound[u, d] + bound[u, target[u]]
        lo = 1 + int((s64[u, d] > s64[u, target[u]] + b).sum())
        hi = 1 + int((s64[u, d] > s64[u, target[u]] - b).sum())
        assert lo <= got[u] <= hi, (u, lo, got[u], hi)
        undecided += lo != hi
    print(f'E = {E}, N = {n}: {undecided} of {prec.shape[0]} users with an undecided pair')
    assert err == 0 and 4 * undecided <= prec.shape[0] and (got > 1).any()


# ------------------------------------------------------------------ 4: exact ranks on integer tables
@pytest.mark.parametrize('sampling', SAMPLINGS)
@pytest.mark.parametrize('E', [64, 128, 256, 512])
def test_exact_ranks_on_integer_tables(E, sampling):
    """Small-integer tables (entries in [-2, 3]): every partial sum is an integer below 2^24, exact in fp32 in any order, and ties are plentiful (the comparison is
    strict: a tie does not beat the target).  Users 0 and 1 keep m = 2 candidates: 100 draws name each many times, and each counts once."""
    U, N1 = 40, 37
    rng = np.random.default_rng(900 + E)
    emb = rng.integers(-2, 3, size=(N1, E)).astype(np.float32)
    prec = rng.integers(-2, 3, size=(U, E)).astype(np.float32)
    cnt = pop_counts(rng, N1, big=False)
    cnt[4], cnt[9], cnt[20] = 3, 1, 5
    cdf = NR.make_cdf(cnt, N1) if sampling == 'pop' else None
    hists = [rng.integers(-1, N1 + 2, size=int(rng.integers(0, 30))) for _ in range(U)]
    target = rng.integers(0, N1 + 1, size=U)
    everything = np.arange(1, N1)
    for u, t in ((0, 21), (1, 0)):                                                # D = everything but items 5 and 10 (both of positive count)
        hists[u], target[u] = everything[(everything != 5) & (everything != 10)], t
    emb[5], emb[10], emb[21] = emb[21] + 1, emb[21], emb[21]                      # user 0: item 10 ties with the target, item 5 may beat it
    prec[0] = np.abs(prec[0]) + 1
    keys = rng.integers(0, 2 ** 31, size=U)
    s64 = prec.astype(np.float64) @ emb.astype(np.float64).T
    p, e = dev(prec), dev(emb)
    for n in (3, 100):
        want, want_err = NR.rank_sampled_reference(s64, hists, target, keys, n, SEED, cdf)
        got, err = run_sampled(p, e, hists, target, keys, n, SEED, cdf)
        np.testing.assert_array_equal(got, want)
        assert err == want_err
        ids, _ = run_draw(hists, target, keys, N1, n, SEED, cdf)
        assert set(ids[0].tolist()) <= {5, 10} and set(ids[1].tolist()) <= {5, 10}
        np.testing.assert_array_equal(got, run_lists_on(p, e, hists, target, ids))
    assert set(ids[0].tolist()) == {5, 10} and got[0] == 2 and got[1] == 1       # 100 draws of two items: one beats the target, the tie does not
    ties = sum(int((s64[u, np.unique(ids[u])] == s64[u, target[u]]).sum()) for u in range(U) if 0 < target[u] < N1)
    assert ties > 0 and (got > 2).any()


# ------------------------------------------------------------------ 5: end to end
@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_eval_model_with_eval_negatives_on_an_id_model(sampling, monkeypatch, tmp_path):
    """--eval_negatives 100 on the small ID model, the spec built from the flags as the runners build it.  The numpy side: the restatement's draws
    and the fp64 product of the vectors the user tower handed the kernel give every user an interval [lo, hi] of ranks (the bound of test 3);
    every rank lies inside it, so HR@10 / nDCG@10 lie between the figures of the hi and of the lo ranks -- which coincide, and are then the
    figures exactly, when no user has an undecided pair (at most 5 % may).  The same figures at 7 users a call, and when the file of
    --eval_negatives_out is read back and given to candidate_lists."""
    import argparse
    from test_topk_gpu import _id_model
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.eval_flags import eval_negatives_from_args
    from adapter4rec_amd.data_utils.metrics import (eval_model, eval_ranks, read_candidate_lists, write_eval_negatives)
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    N1, E = emb.shape
    rng = np.random.default_rng(19)
    U, n = 300, 100
    eval_seq, hist = {}, {}
    for u in range(U):
        s = [int(x) for x in rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False)]
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    target = np.array([eval_seq[u][-1] for u in range(U)])
    hl = [hist[u].numpy() for u in range(U)]

    class Log:
        def __init__(self):
            self.lines = []

        def info(self, msg):
            self.lines.append(str(msg))
    flags = argparse.Namespace(eval_negatives=n, eval_neg_sampling=sampling, eval_neg_seed=SEED % 2 ** 63, eval_negatives_out=None)
    spec = eval_negatives_from_args(flags, {u: eval_seq[u][:-1] for u in range(U)}, item_num, Log())
    assert spec.n == n and (spec.counts is None) == (sampling == 'uniform')
    cdf = None if spec.counts is None else NR.make_cdf(spec.counts[1:], N1)
    seen = []
    real = L.eval_rank_sampled
    monkeypatch.setattr(L, 'eval_rank_sampled', lambda prec, *a: (seen.append(prec.clone()), real(prec, *a))[1], raising=False)
    for name in ('eval_rank', 'eval_rank_lists'):
        monkeypatch.setattr(L, name, lambda *a, **k: pytest.fail('another entry called under eval_negatives'), raising=False)
    log = Log()
    hr = eval_model(model, hist, eval_seq, emb, 256, args, item_num, log, 'test', 0, eval_negatives=spec)
    assert int(spec.last_err.item()) == 0 and f'test_eval_negatives   {U} of {U} users' in log.lines
    line = [l for l in log.lines if 'test_results' in l][0]
    got_hr, got_ndcg = (float(x) / 100 for x in line.split()[1:])
    assert abs(got_hr - hr) < 1e-6
    p64 = torch.cat(seen).double().cpu().numpy()
    assert p64.shape == (U, E)
    ranks = eval_ranks(model, hist, eval_seq, emb, 256, args, list(range(U)), eval_negatives=spec).cpu().numpy()
    e64 = emb.double().cpu().numpy()
    s64 = p64 @ e64.T
    bound = E * 2.0 ** -24 * (np.abs(p64) @ np.abs(e64).T)
    ids, err = NR.draw_negatives(hl, target, np.arange(U), N1, n, spec.seed, cdf)
    lo, hi = np.zeros(U, np.int64), np.zeros(U, np.int64)
    for u in range(U):
        d = np.unique(ids[u])
        b = bound[u, d] + bound[u, target[u]]
        lo[u] = 1 + int((s64[u, d] > s64[u, target[u]] + b).sum())
        hi[u] = 1 + int((s64[u, d] > s64[u, target[u]] - b).sum())
    assert err == 0 and (lo <= ranks).all() and (ranks <= hi).all()
    undecided = int((lo != hi).sum())
    print(f'{sampling}: {undecided} of {U} users with an undecided pair')
    assert undecided <= U // 20
    ones = np.ones(U, bool)
    hit_lo, ndcg_lo, _ = LR.hit_ndcg_means(lo, ones)
    hit_hi, ndcg_hi, _ = LR.hit_ndcg_means(hi, ones)
    assert hit_hi - 1e-6 <= got_hr <= hit_lo + 1e-6 and ndcg_hi - 1e-5 <= got_ndcg <= ndcg_lo + 1e-5          # (the log line carries five decimals of a percentage)
    hit, ndcg, _ = LR.hit_ndcg_means(ranks, ones)
    assert abs(hit - got_hr) < 1e-6 and abs(ndcg - got_ndcg) < 1e-5 and 0 < hit < 1
    # 7 users a call: the same line
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '7')
    log7 = Log()
    assert eval_model(model, hist, eval_seq, emb, 256, args, item_num, log7, 'test', 0, eval_negatives=spec) == hr
    assert [l for l in log7.lines if 'test_results' in l] == [line]
    monkeypatch.delenv('A4R_EVAL_USER_BATCH')
    # the written draws are the restatement's, and replay through the list entry
    monkeypatch.undo()
    user_names = [f'U{u}' for u in range(U)]
    item_names = [None] + [f'N{i}' for i in range(1, N1)]
    path = str(tmp_path / 'neg.tsv')
    assert write_eval_negatives(spec, hist, eval_seq, N1, args, user_names, item_names, path, emb.device) == U
    lists = read_candidate_lists(path, user_names, item_names)
    assert lists == {u: ids[u].tolist() for u in range(U)}
    log2 = Log()
    assert eval_model(model, hist, eval_seq, emb, 256, args, item_num, log2, 'test', 0, candidate_lists=lists) == hr
    assert [l for l in log2.lines if 'test_results' in l] == [line]
