"""Test-only numpy restatement of a4r_topk_lists / a4r_eval_rank_lists (include/a4r_user_lists.h): scores in (any float dtype, fp64 for a
reference), lists / ranks out, plus the shared inputs of tests/test_user_lists_{cpu,gpu}.py.

Every user has a list of item ids of its own; its first max_len entries are read, ids outside 1 .. N1-1 are ignored, a repeated id counts once.
  top-K: topk_ref.topk_reference over the user's distinct listed items outside the user's exclusion list.
  rank[u] = 1 + #{distinct i in list(u) : i not in hist(u), score(u, i) > score(u, target[u])} -- the target need not be listed."""
import numpy as np
import torch

from topk_ref import MAX_EXCL, topk_reference

LIST_MAX = 4096


def listed(ids, N1, max_len=LIST_MAX):
    """the distinct items of a list the kernels honour, ascending"""
    x = np.asarray(list(ids)[:max(int(max_len), 0)], np.int64).reshape(-1)
    return np.unique(x[(x > 0) & (x < N1)])


def _excluded(ids, N1):
    x = np.asarray(list(ids)[:MAX_EXCL], np.int64).reshape(-1)
    return x[(x > 0) & (x < N1)]


def topk_lists_reference(scores, lists, excl_lists, k, max_len=LIST_MAX):
    """scores [U, N1]; lists[u], excl_lists[u]: iterables of ids -> (ids int64 [U, k], scores [U, k]) as topk_reference returns them: per user the
    table is cut down to the pad row and the user's distinct listed rows (ascending, so ties by smaller id are kept), the exclusion list is
    renumbered, and the ids are mapped back."""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    ids = np.zeros((U, k), np.int64)
    out = np.full((U, k), -np.inf, scores.dtype)
    for u in range(U):
        rows = np.concatenate([[0], listed(lists[u], N1, max_len)]).astype(np.int64)
        new = np.zeros(N1, np.int64)
        new[rows] = np.arange(rows.size)
        x = new[_excluded(excl_lists[u], N1)]
        i, v = topk_reference(scores[u:u + 1, rows], [x[x > 0]], k)
        ids[u], out[u] = rows[i[0]], v[0]
    return ids, out


def rank_lists_reference(scores, target, lists, hist_lists, max_len=LIST_MAX):
    """-> ranks int64 [U]"""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    out = np.zeros(U, np.int64)
    for u in range(U):
        items = np.setdiff1d(listed(lists[u], N1, max_len), _excluded(hist_lists[u], N1))
        out[u] = 1 + int((scores[u, items] > scores[u, int(target[u])]).sum())
    return out


def csr_tail(lists, spare=0):
    """-> (ptr int32 [U + 1], flat int32) with nothing behind the last list but ``spare`` zeros (spare = 0: an empty flat array where every list
    is empty)"""
    lens = [len(x) for x in lists]
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in lists] + [np.zeros(spare, np.int64)])
    return ptr.astype(np.int32), flat.astype(np.int32)


def hit_ndcg_means(ranks, has_list, k=10):
    """eval_model's figures under candidate lists: means over the users who have a list -> (hit, ndcg, number of such users)."""
    ranks = np.asarray(ranks, np.float64)
    valid = np.asarray(has_list, bool)
    n = int(valid.sum())
    hit = (ranks <= k) & valid
    ndcg = np.where(hit, 1.0 / np.log2(ranks + 1.0), 0.0)
    return hit.sum() / n, ndcg.sum() / n, n


# ------------------------------------------------------------------ sim_lib-shaped stand-ins for the two wrappers
def _split(ptr, idx, U):
    p = ptr.cpu().numpy().astype(np.int64)
    f = idx.cpu().numpy().astype(np.int64)
    return [f[p[u]:p[u + 1]] for u in range(U)]


def sim_topk_lists(prec, item_emb, list_ptr, list_idx, max_len, excl_ptr, excl_idx, k, ids, scores):
    s = (prec.float() @ item_emb.float().t()).cpu().numpy()
    U = s.shape[0]
    i, v = topk_lists_reference(s, _split(list_ptr, list_idx, U), _split(excl_ptr, excl_idx, U), int(k), max_len)
    ids.copy_(torch.from_numpy(i.astype(np.int32)))
    scores.copy_(torch.from_numpy(v.astype(np.float32)))
    return ids, scores


def sim_eval_rank_lists(prec, item_emb, target, list_ptr, list_idx, max_len, hist_ptr, hist_idx, rank):
    s = (prec.float() @ item_emb.float().t()).cpu().numpy()
    U = s.shape[0]
    r = rank_lists_reference(s, target.cpu().numpy(), _split(list_ptr, list_idx, U), _split(hist_ptr, hist_idx, U), max_len)
    rank.copy_(torch.from_numpy(r.astype(np.int32)))
    return rank


# ------------------------------------------------------------------ the random-table case held against fp64 (tests/test_user_lists_gpu.py)
RANDOM_CASE = dict(seed=31, U=48, N1=4099, K=10, lengths=(0, 1, 5, 9, 10, 11, 64, 200, 257, 1000, 4095, 4096))
RANDOM_E = (64, 128, 512)


def random_case(E):
    """Standard-normal fp32 tables; list lengths cycling through RANDOM_CASE['lengths'], drawn with repeats, pad and out-of-range ids; exclusion
    lists empty, of 264 ids, or short -> (prec, emb, lists, excl, target)."""
    c = RANDOM_CASE
    rng = np.random.default_rng(c['seed'])
    emb = rng.standard_normal((c['N1'], E)).astype(np.float32)
    prec = rng.standard_normal((c['U'], E)).astype(np.float32)
    lists, excl = [], []
    for u in range(c['U']):
        n = c['lengths'][u % len(c['lengths'])]
        lists.append(rng.integers(-2, c['N1'] + 3, size=n))
        m = (0, 264, int(rng.integers(1, 40)))[u % 3]
        excl.append(rng.integers(-3, c['N1'] + 5, size=m))
    target = rng.integers(1, c['N1'], size=c['U'])
    return prec, emb, lists, excl, target


def fp64_reference(prec, emb, lists, excl, k):
    """The fp64 side of the random-table case: scores, the fp32 summation bound E * 2^-24 * sum |a b| per (user, item), the reference lists with
    one position more than k, and per position whether the gap rule makes it sure: an item sits there (pad slots decide nothing and are left
    out of the count) and is separated from both neighbours by more than the user's largest bound.  -> (s64, bound, ri, rs, sure, real)"""
    p, e = prec.astype(np.float64), emb.astype(np.float64)
    s64 = p @ e.T
    bound = prec.shape[1] * 2.0 ** -24 * (np.abs(p) @ np.abs(e).T)
    ri, rs = topk_lists_reference(s64, lists, excl, k + 1)
    sure = np.zeros((prec.shape[0], k), bool)
    for u in range(prec.shape[0]):
        with np.errstate(invalid='ignore'):
            sep = np.concatenate([[True], -np.diff(rs[u]) > bound[u].max()])       # (-inf - -inf = nan: not separated)
        sure[u] = sep[:k] & sep[1:k + 1]
    real = ri[:, :k] != 0
    return s64, bound, ri, rs, sure & real, real
