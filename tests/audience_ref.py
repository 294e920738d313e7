"""Test-only fp64 restatement of the audience rule (include/a4r_audience.h: a4r_topk_users) and a sim_lib-shaped stand-in for _lib.topk_users built
on the same selection.

The rule, restated once:
  score          s(q, r) = <item[q], users[r]>.
  never listed   row 0; a row with elig[r] == 0; a row r whose seen list seen_idx[seen_ptr[r] .. seen_ptr[r + 1]) contains q.
  pad lists      a query id outside 1 .. N1-1: row 0 / -inf in every slot.  Repeated query ids: equal rows.
  order          score descending, ties to the smaller row; short lists end in pads; -0 is returned as +0 (similar_ref.select).
Written in torch so that the larger cases of tests/test_audience_gpu.py can run it on the device (fp64 there too); it returns numpy arrays."""
import numpy as np
import torch

import similar_ref as SR
from similar_ref import decided, integer_table      # noqa: F401  (the audience tests take them from here)


def csr(lists):
    """lists[r]: the seen ids of user-table row r, as given (the caller sorts) -> (ptr int64 [len + 1], flat int32)"""
    lens = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, flat


def csr_of_mask(mask):
    """mask bool [U1, N1]: row r has seen item i -> the CSR of ascending lists (row 0's list is kept as the mask gives it)"""
    return csr([np.flatnonzero(m) for m in np.asarray(mask)])


def seen_matrix(ptr, flat, query, U1):
    """bool numpy [Q, U1]: [j, r] = query[j] is in row r's seen list -- by membership, whatever the list's order"""
    ptr, flat = np.asarray(ptr, dtype=np.int64), np.asarray(flat, dtype=np.int64)
    rows = np.repeat(np.arange(U1), np.diff(ptr[:U1 + 1]))
    body = flat[ptr[0]:ptr[U1]]
    out = np.zeros((len(query), U1), bool)
    for j, q in enumerate(np.asarray(query, dtype=np.int64)):
        out[j, rows[body == q]] = True
    return out


def _select(s, query, n1, listable, k):
    """similar_ref.select on [Q, U1] scores of another table: a column is appended that nothing lists, and a live query is given that column's
    index as its 'self' (select drops the query's own column), a dead one 0 (select pads it)."""
    Q, U1 = s.shape
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(s.device)
    live = (q >= 1) & (q < n1)
    s1 = torch.cat([s, torch.zeros(Q, 1, dtype=s.dtype, device=s.device)], 1)
    ok = torch.cat([listable, torch.zeros(Q, 1, dtype=torch.bool, device=s.device)], 1)
    return SR.select(s1, torch.where(live, torch.full_like(q, U1), torch.zeros_like(q)), ok, int(k))


def scores64(item, users, query):
    """fp64 [Q, U1]: <item[q], users[r]> for the query ids (clamped into the table: dead queries are the selection's)"""
    t = torch.as_tensor(item).double()
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(t.device)
    qc = torch.where((q >= 1) & (q < t.shape[0]), q, torch.zeros_like(q))
    return t[qc] @ torch.as_tensor(users).double().to(t.device).t()


def audience_reference(item, users, query, k, ptr, flat, elig=None):
    """The rule in fp64 -> (rows int64 [Q, k], scores float64 [Q, k]) numpy.  item [N1, E], users [U1, E]: tensors on one device; query: integer
    ids [Q]; ptr / flat: the seen lists' CSR (numpy or tensors); elig: None or [U1] (non-zero = eligible)."""
    item, users = torch.as_tensor(item), torch.as_tensor(users)
    query = np.asarray(query.cpu() if isinstance(query, torch.Tensor) else query, dtype=np.int64)
    np_ = lambda x: np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    U1 = users.shape[0]
    s = scores64(item, users, query)
    ok = ~torch.from_numpy(seen_matrix(np_(ptr), np_(flat), query, U1)).to(s.device)
    if elig is not None:
        ok = ok & torch.from_numpy(np_(elig) != 0).to(s.device)[None, :]
    i, v = _select(s, query, item.shape[0], ok, k)
    return i.cpu().numpy(), v.cpu().numpy()


def bounds(item, users, query):
    """b(q, r) fp64 numpy [Q, U1] = E 2^-24 sum_e |item[q][e] users[r][e]|: the classical bound on the fp32 dot of E products against fp64"""
    t = torch.as_tensor(item).double()
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(t.device)
    return (t.shape[1] * 2.0 ** -24 * (t[q].abs() @ torch.as_tensor(users).double().to(t.device).abs().t())).cpu().numpy()


# (K, E, U1, Q, seed) of the random cases of tests/test_audience_gpu.py; tests/test_audience_cpu.py holds their decided shares
RANDOM_CASES = [(10, 64, 4097, 64, 1), (100, 128, 4097, 64, 2), (256, 64, 2049, 48, 3), (32, 256, 4097, 64, 4), (10, 512, 4097, 64, 5)]
RANDOM_N1 = 257


def random_case(K, E, U1, Q, seed):
    """Standard normal tables (257 items), Q distinct query items, a seen mask of density 0.08 -- and on top of it the 3 K best rows of the
    first query have seen it (the popular-item case) -> item, users (fp32 numpy), query, mask bool [U1, N1]"""
    rng = np.random.default_rng(seed)
    item = rng.standard_normal((RANDOM_N1, E)).astype(np.float32)
    users = rng.standard_normal((U1, E)).astype(np.float32)
    query = rng.permutation(np.arange(1, RANDOM_N1))[:Q]
    mask = rng.random((U1, RANDOM_N1)) < 0.08
    s0 = item[query[0]].astype(np.float64) @ users[1:].astype(np.float64).T
    mask[1 + np.argsort(-s0, kind='stable')[:3 * K], query[0]] = True
    return item, users, query, mask


# ------------------------------------------------------------------ the simulated library's entry (fp32 on the host, the same selection)
def sim_topk_users(item_emb, query, user_vec, seen_ptr, seen_idx, elig, k, rows, scores):
    """_lib.topk_users' stand-in: fp32 dots by torch, the listing rules by membership, selection by similar_ref.select"""
    emb = item_emb.float()
    q = query.long()
    qc = torch.where((q >= 1) & (q < emb.shape[0]), q, torch.zeros_like(q))
    s = emb[qc] @ user_vec.float().t()
    ok = ~torch.from_numpy(seen_matrix(seen_ptr.cpu().numpy(), seen_idx.cpu().numpy(), q.cpu().numpy(), user_vec.shape[0]))
    if elig is not None:
        ok = ok & (elig != 0)[None, :]
    i, v = _select(s, q.cpu().numpy(), emb.shape[0], ok, int(k))
    rows.copy_(i.to(torch.int32))
    scores.copy_(v)
    return rows, scores
