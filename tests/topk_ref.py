"""Test-only numpy restatement of a4r_topk_items (include/a4r.h) and a sim_lib-shaped stand-in for _lib.topk_items built on it.

Semantics restated once: candidates are items 1 .. N1-1 outside the user's exclusion list (ids 0 or >= N1 ignored, repeats count once, at most
A4R_EVAL_MAX_HISTORY ids read); ordered by score descending, ties by smaller id, NaN after every number; short lists end in id 0 / -inf."""
import numpy as np
import torch

MAX_EXCL = 264


def topk_reference(scores, excl_lists, k):
    """scores: float array [U, N1] (row u = the user's score of every table row); excl_lists[u]: iterable of ids.
    -> (ids int64 [U, k], scores [U, k] of scores' dtype)."""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    ids = np.zeros((U, k), np.int64)
    out = np.full((U, k), -np.inf, scores.dtype)
    for u in range(U):
        cand = np.ones(N1, bool)
        cand[0] = False
        ex = np.asarray(list(excl_lists[u])[:MAX_EXCL], np.int64).reshape(-1)
        cand[ex[(ex > 0) & (ex < N1)]] = False
        c = np.flatnonzero(cand)
        s = scores[u, c]
        nan = np.isnan(s)
        order = np.lexsort((c, -np.where(nan, 0, s), nan))       # primary: numbers before NaN; then score descending; then id ascending
        n = min(k, c.size)
        ids[u, :n] = c[order[:n]]
        out[u, :n] = s[order[:n]]
    out[out == 0] = 0.0                                            # (-0 is returned as +0)
    return ids, out


def csr(lists):
    """-> (ptr int32 [U + 1], flat int32 [>= 1]) as a4r_topk_items reads an exclusion list."""
    lens = [len(x) for x in lists]
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in lists] + [np.zeros(1, np.int64)])
    return ptr.astype(np.int32), flat.astype(np.int32)


def sim_topk_items(prec, item_emb, excl_ptr, excl_idx, k, ids, scores):
    """The simulated library's topk_items: fp32 scores by torch on the host, selection by topk_reference."""
    s = (prec.float() @ item_emb.float().t()).cpu().numpy()
    p = excl_ptr.cpu().numpy().astype(np.int64)
    f = excl_idx.cpu().numpy().astype(np.int64)
    lists = [f[p[u]:p[u + 1]] for u in range(s.shape[0])]
    i, v = topk_reference(s, lists, int(k))
    ids.copy_(torch.from_numpy(i.astype(np.int32)))
    scores.copy_(torch.from_numpy(v.astype(np.float32)))
    return ids, scores
