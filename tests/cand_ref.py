"""Test-only numpy restatement of a4r_eval_rank_cand / a4r_topk_items_cand (include/a4r_candidates.h): scores in (any float dtype, fp64 for a
reference), ranks / lists out, plus the shared inputs of tests/test_candidates_{cpu,gpu}.py.

A candidate set is one entry per table row; item i is a candidate iff cand[i] != 0, cand[0] is ignored.
  rank[u] = 1 + #{i in 1 .. N1-1 : cand[i] != 0, i not in hist(u), score(u, i) > score(u, target[u])} -- the target need not be a candidate.
  top-K: topk_ref.topk_reference over the candidates outside the user's list."""
import numpy as np

from topk_ref import MAX_EXCL, topk_reference


def _listed(ids, N1):
    """the ids of a history / exclusion list the kernels honour: the first MAX_EXCL read, 0 and ids outside the table ignored"""
    x = np.asarray(list(ids)[:MAX_EXCL], np.int64).reshape(-1)
    return x[(x > 0) & (x < N1)]


def rank_cand_reference(scores, target, hist_lists, cand):
    """scores [U, N1]; target [U]; hist_lists[u]: iterable of ids; cand [N1] -> ranks int64 [U]."""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    c = np.asarray(cand).reshape(-1) != 0
    assert c.size == N1
    out = np.zeros(U, np.int64)
    for u in range(U):
        ok = c.copy()
        ok[0] = False
        ok[_listed(hist_lists[u], N1)] = False
        out[u] = 1 + int((scores[u, ok] > scores[u, int(target[u])]).sum())
    return out


def topk_cand_reference(scores, excl_lists, cand, k):
    """-> (ids int64 [U, k], scores [U, k]) as topk_reference returns them.  Extending every user's list by the non-candidates would state the
    same thing, but topk_reference reads a list only up to MAX_EXCL ids, as the kernel does: here the table is cut down to the pad row and the
    candidate rows instead (ascending, so ties by smaller id are kept), the users' lists are renumbered, and the ids are mapped back."""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    c = np.asarray(cand).reshape(-1) != 0
    assert c.size == N1
    rows = np.concatenate([[0], np.flatnonzero(c[1:]) + 1])          # kept table rows: the pad row first
    new = np.zeros(N1, np.int64)
    new[rows] = np.arange(rows.size)
    lists = []
    for u in range(U):
        x = new[_listed(excl_lists[u], N1)]
        lists.append(x[x > 0])
    ids, out = topk_reference(scores[:, rows], lists, k)
    return rows[ids], out


def hit_ndcg_means(ranks, target, cand, k=10):
    """eval_model's figures under a candidate set: means over the users whose target is a candidate -> (hit, ndcg, number of such users)."""
    ranks = np.asarray(ranks, np.float64)
    valid = np.asarray(cand).reshape(-1)[np.asarray(target, np.int64)] != 0
    n = int(valid.sum())
    hit = (ranks <= k) & valid
    ndcg = np.where(hit, 1.0 / np.log2(ranks + 1.0), 0.0)
    return hit.sum() / n, ndcg.sum() / n, n


# ------------------------------------------------------------------ the random-table case held against fp64 (tests/test_candidates_gpu.py)
RANDOM_CASE = dict(seed=20, U=64, N1=65537, E=64, K=10, fraction=0.5)


def random_case():
    """Standard-normal fp32 tables, a mask at 0.5 and exclusion lists with repeats, pad and out-of-range ids -> (prec, emb, cand, lists, targets)."""
    c = RANDOM_CASE
    rng = np.random.default_rng(c['seed'])
    emb = rng.standard_normal((c['N1'], c['E'])).astype(np.float32)
    prec = rng.standard_normal((c['U'], c['E'])).astype(np.float32)
    cand = (rng.random(c['N1']) < c['fraction']).astype(np.uint8)
    lists = []
    for u in range(c['U']):
        n = (0, 264, int(rng.integers(1, 40)))[u % 3]
        x = rng.integers(-3, c['N1'] + 5, size=n)
        if n:
            x[: n // 4] = x[n // 4: 2 * (n // 4)]
            x[-1] = 0
        lists.append(x)
    target = rng.integers(1, c['N1'], size=c['U'])
    return prec, emb, cand, lists, target


def fp64_reference(prec, emb, cand, lists, k):
    """The fp64 side of the random-table case: scores, the fp32 summation bound E * 2^-24 * sum |a b| per (user, item), the reference lists with
    one position more than k, and per position whether the gap rule makes it sure (separated from both neighbours by more than the user's
    largest bound)."""
    p, e = prec.astype(np.float64), emb.astype(np.float64)
    s64 = p @ e.T
    bound = prec.shape[1] * 2.0 ** -24 * (np.abs(p) @ np.abs(e).T)
    ri, rs = topk_cand_reference(s64, lists, cand, k + 1)
    sure = np.zeros((prec.shape[0], k), bool)
    for u in range(prec.shape[0]):
        sep = np.concatenate([[True], -np.diff(rs[u]) > bound[u].max()])
        sure[u] = sep[:k] & sep[1:k + 1]
    return s64, bound, ri, rs, sure
