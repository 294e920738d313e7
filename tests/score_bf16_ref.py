"""Test-only fp64 restatement of a4r_eval_rank_bf16 / a4r_topk_items_bf16 (include/a4r_score_bf16.h), the shared inputs of
tests/test_score_bf16_{cpu,gpu}.py, and sim_lib-shaped stand-ins for the two wrappers.

The rule: prec_b = bf16(prec), table_b = bf16(item_emb), rounded to nearest even on the bit pattern (score_ce_bf16_ref.round_bf16, what
a4r_score_ce_bf16_cast does); score(u, i) = <prec_b[u], table_b[i]>.  Everything else is the fp32 entries' contract, restated in topk_ref.py and
cand_ref.py and applied here to the scores of the rounded operands:
  rank[u] = 1 + #{i in 1 .. N1-1 : (cand is None or cand[i] != 0), i not in hist(u), score(u, i) > score(u, target[u])}
  top-K   = topk_ref.topk_reference over the items (the candidates) outside the user's list.
The products of two bf16 numbers are exact in fp32 (8 + 8 significand bits) and the kernels add them in fp32, so a kernel score lies within the
classical recursive-summation bound  E x 2^-24 x sum_k |a_k b_k|  of the fp64 score at the SAME rounded operands: the bound the fp32 tests use."""
import numpy as np
import torch

from cand_ref import rank_cand_reference, topk_cand_reference
from score_ce_bf16_ref import round_bf16
from topk_ref import topk_reference


def rounded(x):
    """fp32 array -> the bf16-rounded values as fp64"""
    return round_bf16(np.asarray(x, np.float32)).astype(np.float64)


def scores64(prec, emb):
    """fp64 scores [U, N1] at the rounded operands"""
    return rounded(prec) @ rounded(emb).T


def sum_bound(prec, emb):
    """E x 2^-24 x sum |a b| per (user, item) at the rounded operands"""
    return prec.shape[1] * 2.0 ** -24 * (np.abs(rounded(prec)) @ np.abs(rounded(emb)).T)


def rank_reference(scores, target, hist_lists, cand=None):
    scores = np.asarray(scores)
    return rank_cand_reference(scores, target, hist_lists, np.ones(scores.shape[1], np.uint8) if cand is None else cand)


def topk_reference_cand(scores, excl_lists, k, cand=None):
    return topk_reference(scores, excl_lists, k) if cand is None else topk_cand_reference(scores, excl_lists, cand, k)


def rank_interval(s64, bound, target, hist_lists, cand=None):
    """-> (lo, hi) int64 [U]: 1 + the count of valid items whose fp64 score exceeds the target's by more than +2b / -2b, b the user's largest
    summation bound (an item's and the target's kernel scores each lie within b of fp64)."""
    U, N1 = s64.shape
    c = np.ones(N1, bool) if cand is None else np.asarray(cand).reshape(-1) != 0
    lo, hi = np.zeros(U, np.int64), np.zeros(U, np.int64)
    for u in range(U):
        ok = c.copy()
        ok[0] = False
        x = np.asarray(list(hist_lists[u])[:264], np.int64).reshape(-1)
        ok[x[(x > 0) & (x < N1)]] = False
        b, t = bound[u].max(), s64[u, int(target[u])]
        lo[u] = 1 + int((s64[u, ok] > t + 2 * b).sum())
        hi[u] = 1 + int((s64[u, ok] > t - 2 * b).sum())
    return lo, hi


def hit_ndcg(ranks, k=10):
    """eval_model's two means over all users, in fp64"""
    r = np.asarray(ranks, np.float64)
    hit = r <= k
    return float(hit.mean()), float(np.where(hit, 1.0 / np.log2(r + 1.0), 0.0).mean())


# ------------------------------------------------------------------ shared inputs
def excl_lists(rng, U, N1):
    """0 ids, 264 ids with repeats, pad / negative / out-of-range ids, everything in between (tests/test_topk_gpu.py's lists)."""
    out = []
    for u in range(U):
        n = (0, 264, int(rng.integers(1, 40)))[u % 3]
        x = rng.integers(-3, N1 + 5, size=n)
        if n:
            x[: n // 4] = x[n // 4: 2 * (n // 4)]
            x[-1] = 0
        out.append(x)
    return out


def integer_case(seed, U, N1, E):
    """Tables of integers in [-8, 8] (exact in bf16; every score is an integer below 2^24, exact in fp32 whatever the summation order), with
    duplicated rows and all-zero users -> (prec fp32 [U, E], emb fp32 [N1, E], lists, target)."""
    rng = np.random.default_rng(seed)
    emb = rng.integers(-8, 9, size=(N1, E)).astype(np.float32)
    if N1 > 8:
        src = rng.integers(1, N1, size=N1 // 8)
        emb[rng.integers(1, N1, size=N1 // 8)] = emb[src]
    prec = rng.integers(-8, 9, size=(U, E)).astype(np.float32)
    prec[::5] = 0.0
    return prec, emb, excl_lists(rng, U, N1), rng.integers(1, N1, size=U)


RANDOM_SHAPES = [(10, 64), (100, 128), (256, 512)]      # (K, E) at U = 64, N1 = 65537
RANDOM_U, RANDOM_N1 = 64, 65537
_RANDOM = {}


def random_case(K, E):
    """Standard-normal fp32 tables and the fp64 side at the rounded operands, computed once per shape and shared (never written to):
    dict(prec, emb, lists, target, s64, bound, ri, rs (K + 1 positions), sure [U, K]: the gap rule -- a position is compared when separated from
    both neighbours by more than the user's largest bound)."""
    if (K, E) not in _RANDOM:
        rng = np.random.default_rng(K + E)
        emb = rng.standard_normal((RANDOM_N1, E)).astype(np.float32)
        prec = rng.standard_normal((RANDOM_U, E)).astype(np.float32)
        lists = excl_lists(rng, RANDOM_U, RANDOM_N1)
        target = rng.integers(1, RANDOM_N1, size=RANDOM_U)
        s64, bound = scores64(prec, emb), sum_bound(prec, emb)
        ri, rs = topk_reference(s64, lists, K + 1)
        sure = np.zeros((RANDOM_U, K), bool)
        for u in range(RANDOM_U):
            sep = np.concatenate([[True], -np.diff(rs[u]) > bound[u].max()])
            sure[u] = sep[:K] & sep[1:K + 1]
        _RANDOM[(K, E)] = dict(prec=prec, emb=emb, lists=lists, target=target, s64=s64, bound=bound, ri=ri, rs=rs, sure=sure)
    return _RANDOM[(K, E)]


# ------------------------------------------------------------------ stand-ins for the wrappers (CPU tests: the simulated library)
def _csr_lists(ptr, idx, U):
    p, f = ptr.cpu().numpy().astype(np.int64), idx.cpu().numpy().astype(np.int64)
    return [f[p[u]:p[u + 1]] for u in range(U)]


def _operands64(prec_b, table_b):
    assert prec_b.dtype == torch.bfloat16 and table_b.dtype == torch.bfloat16 and prec_b.is_contiguous() and table_b.is_contiguous()
    return prec_b.double().cpu().numpy(), table_b.double().cpu().numpy()         # (bf16 -> fp64 is exact)


def sim_eval_rank_bf16(prec_b, table_b, target, hist_ptr, hist_idx, rank, cand=None):
    p, t = _operands64(prec_b, table_b)
    c = None if cand is None else cand.cpu().numpy()
    r = rank_reference(p @ t.T, target.cpu().numpy(), _csr_lists(hist_ptr, hist_idx, p.shape[0]), c)
    rank.copy_(torch.from_numpy(r.astype(np.int32)))


def sim_topk_items_bf16(prec_b, table_b, excl_ptr, excl_idx, k, ids, scores, cand=None):
    p, t = _operands64(prec_b, table_b)
    c = None if cand is None else cand.cpu().numpy()
    i, v = topk_reference_cand(p @ t.T, _csr_lists(excl_ptr, excl_idx, p.shape[0]), int(k), c)
    ids.copy_(torch.from_numpy(i.astype(np.int32)))
    scores.copy_(torch.from_numpy(v.astype(np.float32)))
    return ids, scores


def sim_cast_bf16(src, dst, n=None):
    """_lib_ce_bf16.cast_bf16 on the host: round_bf16 on the bit pattern"""
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.is_contiguous() and dst.is_contiguous()
    r = torch.from_numpy(round_bf16(src.detach().cpu().numpy().reshape(-1))).to(torch.bfloat16)        # (exact: the values are bf16 already)
    dst.view(-1)[:r.numel() if n is None else n].copy_(r[:r.numel() if n is None else n])
