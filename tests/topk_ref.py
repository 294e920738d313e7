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


TRIGGER_N1, TRIGGER_U = 4097, 32769


def trigger_case(E):
    """The input that drives the top-K kernels' append-and-trigger path at its bound (random tables raise the thresholds within a few tiles, after
    which a step rarely adds a key).  Table: 256 tiles of 16 items, emb[i, 0] = the tile of item i, every other column 0 -- integers up to 255,
    exact in bf16, every score exact in fp32.  32769 users: more than 2048 workgroups, so one item range, 64 steps of 4 tiles per workgroup, and
    a partial last workgroup (or row set).  Three classes by u % 3, prec[u, 0] = 1 / -1 / 0: scores ascend with the tile, so all 64 lane columns
    of every step beat the threshold (64 appends per user and step but for the excluded ids: at cap = 128 every step compacts) / scores descend,
    nothing is appended after the first steps / every score ties and the order falls to the ids.  One exclusion list per class, each with ids of the
    highest tiles; the first is full (264 ids) with repeats and ids outside the table.
    -> (emb fp32 [N1, E], prec fp32 [U, E], the three lists)."""
    N1, U = TRIGGER_N1, TRIGGER_U
    emb = np.zeros((N1, E), np.float32)
    emb[1:, 0] = (np.arange(1, N1) - 1) // 16
    prec = np.zeros((U, E), np.float32)
    prec[:, 0] = np.array([1.0, -1.0, 0.0], np.float32)[np.arange(U) % 3]
    top = np.arange(N1 - 1, N1 - 401, -2)                          # every other id of the 25 highest tiles
    lists = [np.concatenate([top, top[:60], [0, -3, N1, N1 + 7]]),
             np.array([1, 2, 16, 17, 40, N1 - 1, N1 - 2, N1 - 16, N1 - 17, 0]),
             np.array([N1 - 1, 3, 1, 5, 64, 65, N1 - 5, 3])]
    assert len(lists[0]) == MAX_EXCL
    return emb, prec, lists


def trigger_expected(emb, prec, lists, k):
    """The lists of trigger_case's users: one per class by topk_reference, broadcast -> (ids int64 [U, k], scores fp32 [U, k])"""
    s = (prec[:3].astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32)      # exact
    ids, sc = topk_reference(s, lists, k)
    cls = np.arange(prec.shape[0]) % 3
    return ids[cls], sc[cls]


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
