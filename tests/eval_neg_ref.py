"""The draw rule of a sampled evaluation's negatives (include/a4r_eval_negatives.h) restated on the CPU: the counter hash of
oracle/dropout_masks.py, a 128-bit product in Python ints and the SEQUENTIAL walk over the user's sorted distinct ids (the kernels search instead:
they must give these ids).  Shared by the CPU tests (properties of the rule, eval_model on the stand-in library) and the GPU tests (the kernels
must give these bits).  Ranks come from lists_ref.rank_lists_reference on the drawn ids."""
import numpy as np
import torch

import lists_ref as LR
from oracle.dropout_masks import hash64

EVAL_NEG_SITE = 7002        # A4R_EVAL_NEG_SITE (include/a4r_eval_negatives.h)
MAX_HISTORY = 264           # A4R_EVAL_MAX_HISTORY (include/a4r.h)
NEG_MAX = 4096              # A4R_LIST_MAX


def make_cdf(counts, N1):
    """counts: N1 - 1 non-negative ints (item 1 .. N1-1) -> Python-int list cdf[N1], cdf[0] = 0"""
    counts = [int(c) for c in counts]
    assert len(counts) == N1 - 1 and all(c >= 0 for c in counts)
    cdf = [0] * N1
    for i, c in enumerate(counts, 1):
        cdf[i] = cdf[i - 1] + c
    assert cdf[-1] < 2 ** 63
    return cdf


def exclusion_set(hist, target, N1):
    """D(u): the distinct ids in 1 .. N1-1 among the first MAX_HISTORY ids of the history, and the target if it is an item, ascending"""
    ids = [int(x) for x in list(hist)[:MAX_HISTORY]] + [int(target)]
    return sorted({x for x in ids if 0 < x < N1})


def user_draws(hist, target, uk, N1, n, seed, cdf=None):
    """-> (n drawn ids as an int64 array, m).  cdf: None = uniform, or make_cdf's list.  m < 1: zeros.  The product is taken in Python ints; the
    walk runs over D in sequence, on all n draws at once (every value stays below cdf[N1 - 1] < 2^63)."""
    assert 1 <= n <= NEG_MAX and N1 >= 2 and -2 ** 31 <= int(uk) < 2 ** 31
    c = (lambda i: i) if cdf is None else (lambda i: cdf[i])
    D = exclusion_set(hist, target, N1)
    m = c(N1 - 1) - sum(c(s) - c(s - 1) for s in D)
    if m < 1:
        return np.zeros(n, np.int64), m
    key = (int(uk) & 0xFFFFFFFF) << 16
    h = hash64(seed, EVAL_NEG_SITE, np.array([key | j for j in range(n)], dtype=np.uint64))
    x = np.array([(int(hv) * m) >> 64 for hv in h], dtype=np.int64)               # the high half of the 64 x 64-bit product
    for s in D:
        x += np.where(x >= c(s - 1), c(s) - c(s - 1), 0).astype(np.int64)
    if cdf is None:
        return x + 1, m
    ids = np.searchsorted(np.asarray(cdf, np.int64), x, side='right')              # the smallest i with cdf[i] > x
    return ids.astype(np.int64), m


def draw_negatives(hists, target, user_key, N1, n, seed, cdf=None):
    """-> (ids int64 [U, n], err = the users without a candidate)"""
    U = len(target)
    out = np.zeros((U, n), np.int64)
    err = 0
    for u in range(U):
        out[u], m = user_draws(hists[u], target[u], user_key[u], N1, n, seed, cdf)
        err += m < 1
    return out, int(err)


def rank_sampled_reference(scores, hists, target, user_key, n, seed, cdf=None):
    """scores [U, N1] (any float dtype) -> (ranks int64 [U], err): rank_lists_reference on the drawn ids; a target that is no item gets rank 1"""
    scores = np.asarray(scores)
    U, N1 = scores.shape
    ids, err = draw_negatives(hists, target, user_key, N1, n, seed, cdf)
    t = np.asarray(target, np.int64)
    is_item = (t > 0) & (t < N1)
    ranks = LR.rank_lists_reference(scores, np.where(is_item, t, 0), [ids[u] for u in range(U)], hists)
    return np.where(is_item, ranks, 1), err


# ------------------------------------------------------------------ stand-ins of the two wrappers (host tensors) for the CPU runs
def _split(ptr, idx, U):
    p = ptr.cpu().numpy().astype(np.int64)
    f = idx.cpu().numpy().astype(np.int64)
    return [f[p[u]:p[u + 1]] for u in range(U)]


def _cdf_list(cdf):
    return None if cdf is None else [int(x) for x in cdf.cpu().numpy()]


def sim_eval_draw_negatives(hist_ptr, hist_idx, target, user_key, cdf, seed, n1, out_ids, err):
    U, n = out_ids.shape
    ids, e = draw_negatives(_split(hist_ptr, hist_idx, U), target.cpu().numpy(), user_key.cpu().numpy(), int(n1), n, seed, _cdf_list(cdf))
    out_ids.copy_(torch.from_numpy(ids.astype(np.int32)))
    err += e
    return out_ids


def sim_eval_rank_sampled(prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, seed, n, rank, err):
    s = (prec.float() @ item_emb.float().t()).cpu().numpy()
    U = s.shape[0]
    r, e = rank_sampled_reference(s, _split(hist_ptr, hist_idx, U), target.cpu().numpy(), user_key.cpu().numpy(), int(n), seed, _cdf_list(cdf))
    rank.copy_(torch.from_numpy(r.astype(np.int32)))
    err += e
    return rank
