"""Test-only numpy restatement of a4r_topk_items_excl (include/a4r_exclude.h) on top of topk_ref.topk_reference, an int64-offset CSR builder
and a sim_lib-shaped stand-in for _lib.topk_items_excl.

The rule restated once: a4r_topk_items' rule (topk_ref) with a user's exclusion list of any length -- no 264-id cap -- and, under a candidate
mask, only the items i with cand[i] != 0.  Repeated ids, id 0 and ids outside 1 .. N1-1 match nothing."""
import numpy as np
import torch

from topk_ref import topk_reference


def excl_reference(scores, excl_lists, k, cand=None):
    """scores: float array [U, N1]; excl_lists[u]: iterable of ids, of any length; cand: None or [N1], non-zero = a candidate.
    -> (ids int64 [U, k], scores [U, k] of scores' dtype).  topk_reference orders the columns that are left (listed and non-candidate items are
    cut out of the row; the map back to ids is monotone, so ties keep their order by id)."""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    ids = np.zeros((U, k), np.int64)
    out = np.full((U, k), -np.inf, scores.dtype)
    keep = np.ones(N1, bool) if cand is None else np.asarray(cand).reshape(-1) != 0
    for u in range(U):
        ok = keep.copy()
        ex = np.asarray(list(excl_lists[u]), np.int64).reshape(-1)
        ok[ex[(ex > 0) & (ex < N1)]] = False
        ok[0] = False
        c = np.flatnonzero(ok)                                       # the user's candidates, ascending
        i, s = topk_reference(scores[u:u + 1, np.concatenate([[0], c])], [[]], k)      # (column 0 stands for the pad row)
        n = int((i[0] != 0).sum())
        ids[u, :n] = c[i[0, :n] - 1]
        out[u, :n] = s[0, :n]
    return ids, out


def csr64(lists, sort=True):
    """-> (ptr int64 [U + 1], flat int32 [>= 1]) as a4r_topk_items_excl reads the lists: each user's ids ascending (repeats and ids that are no
    item kept: they match nothing), one spare 0 behind the last."""
    rows = [np.asarray(list(x), np.int64).reshape(-1) for x in lists]
    if sort:
        rows = [np.sort(x, kind='stable') for x in rows]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([x.size for x in rows], out=ptr[1:])
    flat = np.concatenate(rows + [np.zeros(1, np.int64)])
    return ptr, flat.astype(np.int32)


def lists_of_csr(excl_ptr, excl_idx):
    p = np.asarray(excl_ptr.cpu() if isinstance(excl_ptr, torch.Tensor) else excl_ptr).astype(np.int64)
    f = np.asarray(excl_idx.cpu() if isinstance(excl_idx, torch.Tensor) else excl_idx).astype(np.int64)
    return [f[p[u]:p[u + 1]] for u in range(p.size - 1)]


def sim_topk_items_excl(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores):
    """The simulated library's topk_items_excl (the wrapper's signature): fp32 scores by torch on the host, selection by excl_reference."""
    s = (prec.float() @ item_emb.float().t()).cpu().numpy()
    i, v = excl_reference(s, lists_of_csr(excl_ptr, excl_idx), int(k), None if cand is None else cand.cpu().numpy())
    ids.copy_(torch.from_numpy(i.astype(np.int32)))
    scores.copy_(torch.from_numpy(v.astype(np.float32)))
    return ids, scores
