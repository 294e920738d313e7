"""Test-only fp64 restatement of the similar-item rule (include/a4r_similar.h: a4r_row_inv_norms, a4r_topk_similar) and sim_lib-shaped stand-ins
for _lib.row_inv_norms / _lib.topk_similar built on the same selection.

The rule, restated once:
  inverse norm   inv[i] = 1 / sqrt(sum_e x[i][e]^2), 0 when that sum is 0 or not finite (a zero row, a row holding inf or NaN); every row, row 0 too.
  score          dot:  s(q, i) = <x[q], x[i]>;   cos:  s(q, i) = <x[q], x[i]> * (inv[q] * inv[i]), the product of the two inverse norms first.
  never listed   row 0, the query itself, an item with cand[i] == 0, (cos) an item with inv[i] == 0, an item whose score is not >= min_sim (a NaN
                 score is never listed; -inf = no floor).
  pad lists      a query id outside 1 .. N1-1, and (cos) a query with inv[q] == 0: id 0 / -inf in every slot.  Repeated query ids: equal rows.
  order          score descending, ties to the smaller id; short lists end in pads; -0 is returned as +0.
Written in torch so that the large cases of tests/test_similar_gpu.py can run it on the device (fp64 there too); it returns numpy arrays."""
import numpy as np
import torch


def inv_norms64(table):
    """fp64 tensor [N1]: the inverse norms of the rule, before any rounding."""
    t = table.double()
    ss = (t * t).sum(1)
    ok = (ss > 0) & torch.isfinite(ss)
    return torch.where(ok, 1.0 / torch.sqrt(torch.where(ok, ss, torch.ones_like(ss))), torch.zeros_like(ss))


def inv_norms_reference(table):
    """a4r_row_inv_norms restated: fp32 numpy [N1] = the fp64 inverse norm rounded once."""
    return inv_norms64(torch.as_tensor(table)).to(torch.float32).cpu().numpy()


def select(s, query, listable, k):
    """The selection of the rule on a score matrix.  s [Q, N1] (any float dtype): s[r, i] = score(query[r], i); listable bool [Q, N1]: what the
    rule leaves of metric, candidates and floor (row 0, self, NaN scores and dead queries are taken out here).  -> (ids int64 [Q, k], scores
    [Q, k] of s's dtype) as tensors on s's device."""
    Q, N1 = s.shape
    q = query.to(s.device).long()
    col = torch.arange(N1, device=s.device)
    ok = listable & (col[None, :] >= 1) & (col[None, :] != q[:, None]) & ~torch.isnan(s) & ((q >= 1) & (q < N1))[:, None]
    key = torch.where(ok, -s, torch.full_like(s, float('nan')))                 # ascending, stable: score descending, ties by id, NaN (= not listed) last
    order = torch.sort(key, dim=1, stable=True).indices[:, :k]
    n = ok.sum(1)
    got = torch.gather(s, 1, order)
    pad = torch.arange(order.shape[1], device=s.device)[None, :] >= n[:, None]
    ids = torch.where(pad, torch.zeros_like(order), order)
    sc = torch.where(pad, torch.full_like(got, -float('inf')), got)
    sc = torch.where(sc == 0, torch.zeros_like(sc), sc)                          # -0 is returned as +0
    if order.shape[1] < k:                                                       # k > N1: pads
        ids = torch.cat([ids, torch.zeros(Q, k - order.shape[1], dtype=ids.dtype, device=s.device)], 1)
        sc = torch.cat([sc, torch.full((Q, k - order.shape[1]), -float('inf'), dtype=sc.dtype, device=s.device)], 1)
    return ids, sc


def scores64(table, query, metric='cos'):
    """(s fp64 [Q, N1], listable bool [Q, N1] by the metric alone) for the query ids (clamped into the table: dead queries are select's)."""
    t = table.double()
    N1 = t.shape[0]
    q = query.to(t.device).long()
    qc = torch.where((q >= 1) & (q < N1), q, torch.zeros_like(q))
    s = t[qc] @ t.t()
    if metric == 'dot':
        return s, torch.ones_like(s, dtype=torch.bool)
    inv = inv_norms64(t)
    return s * (inv[qc][:, None] * inv[None, :]), (inv[qc] != 0)[:, None] & (inv != 0)[None, :]


def similar_reference(table, query, k, metric='cos', cand=None, min_sim=None, chunk=2048):
    """The rule in fp64 -> (ids int64 [Q, k], scores float64 [Q, k]) numpy.  table: tensor [N1, E] on any device; query: integer ids [Q];
    cand: None or [N1] (non-zero = candidate); min_sim: None = no floor."""
    table = torch.as_tensor(table)
    query = torch.as_tensor(np.asarray(query, dtype=np.int64) if not isinstance(query, torch.Tensor) else query)
    c = None if cand is None else (torch.as_tensor(np.asarray(cand.cpu() if isinstance(cand, torch.Tensor) else cand)) != 0).to(table.device)
    out_i, out_s = [], []
    for a in range(0, query.numel(), chunk):
        qa = query[a:a + chunk]
        s, ok = scores64(table, qa, metric)
        if c is not None:
            ok = ok & c[None, :]
        if min_sim is not None:
            ok = ok & (s >= float(min_sim))
        i, v = select(s, qa, ok, int(k))
        out_i.append(i.cpu())
        out_s.append(v.cpu())
    return torch.cat(out_i).numpy(), torch.cat(out_s).numpy()


# ------------------------------------------------------------------ the simulated library's entries (fp32 on the host, the same selection)
def sim_row_inv_norms(table, out=None):
    inv = inv_norms64(table).to(torch.float32)
    if out is None:
        return inv
    out.copy_(inv)
    return out


def sim_topk_similar(item_emb, inv_norm, query, cand, min_sim, k, ids, scores):
    """_lib.topk_similar's stand-in: fp32 dots by torch, score = dot * (inv[q] * inv[i]) in fp32 as the kernel forms it, selection by select."""
    emb = item_emb.float()
    N1 = emb.shape[0]
    q = query.long()
    qc = torch.where((q >= 1) & (q < N1), q, torch.zeros_like(q))
    s = emb[qc] @ emb.t()
    ok = torch.ones_like(s, dtype=torch.bool)
    if inv_norm is not None:
        s = s * (inv_norm[qc][:, None] * inv_norm[None, :])
        ok = (inv_norm[qc] != 0)[:, None] & (inv_norm != 0)[None, :]
    if cand is not None:
        ok = ok & (cand != 0)[None, :]
    if min_sim is not None:
        ok = ok & (s >= torch.tensor(float(min_sim), dtype=torch.float32))
    i, v = select(s, q, ok, int(k))
    ids.copy_(i.to(torch.int32))
    scores.copy_(v)
    return ids, scores


# ------------------------------------------------------------------ tables whose scores are exact in fp32
def integer_table(rng, N1, E, dup=True, zero_rows=()):
    """integers in -8 .. 8: every dot product is exact in fp32; an eighth of the rows are copies of other rows (equal scores: ties by id)"""
    t = rng.integers(-8, 9, size=(N1, E)).astype(np.float32)
    if dup and N1 > 8:
        src = rng.integers(1, N1, size=N1 // 8)
        t[rng.integers(1, N1, size=N1 // 8)] = t[src]
    for z in zero_rows:
        t[z] = 0
    return t


def exact_cosine_table(rng, N1, E):
    """every row: exactly 16 non-zero entries +-2^a, one a in -3 .. 3 per row.  The squared norm is 16 * 4^a, the inverse norm 2^-(a + 2), the
    product of two of them a power of two, the dot an integer m times a power of two with |m| <= 16: every step of the kernel is exact and the
    cosine is m / 16, one of 33 values."""
    t = np.zeros((N1, E), np.float32)
    pos = np.argsort(rng.random((N1, E)), axis=1)[:, :16]                       # 16 distinct columns per row
    val = rng.choice(np.array([-1.0, 1.0], np.float32), size=(N1, 16)) * np.exp2(rng.integers(-3, 4, size=(N1, 1))).astype(np.float32)
    np.put_along_axis(t, pos, val, axis=1)
    return t


# ------------------------------------------------------------------ random tables: the error bound and the decided positions
def cosine_bounds(table, query):
    """b(q, i) fp64 numpy [Q, N1] for the cosine the kernel forms in fp32 against the fp64 cosine:
         b = E 2^-24 (|a| . |b|) / (|a| |b|)  +  4 x 2^-24 |cos|
    the classical bound on the fp32 dot of E products, scaled as the score is, plus one rounding each for the two inverse norms, their product
    and the final multiply."""
    t = torch.as_tensor(table).double()
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(t.device)
    inv = inv_norms64(t)
    w = inv[q][:, None] * inv[None, :]
    dot_abs = t[q].abs() @ t.abs().t()
    cos = (t[q] @ t.t()) * w
    return (t.shape[1] * 2.0 ** -24 * dot_abs * w + 4 * 2.0 ** -24 * cos.abs()).cpu().numpy()


def decided(rs, bmax):
    """rs [Q, K + 1]: the restatement's scores at K + 1 depth; bmax [Q]: the largest b of the row.  -> bool [Q, K]: position j is decided when
    its score is separated from both neighbours' by more than 2 bmax (the first position has one neighbour)."""
    with np.errstate(invalid='ignore'):
        gap = -np.diff(rs, axis=1) > 2 * np.asarray(bmax)[:, None]
    sep = np.concatenate([np.ones((rs.shape[0], 1), bool), gap], axis=1)
    return sep[:, :-1] & sep[:, 1:]
