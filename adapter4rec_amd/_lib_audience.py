"""ctypes binding of the audience lists: the a4r_topk_users export of liba4r_hip.so, declared in include/a4r_audience.h (which include/a4r.h
includes).  Same rules as adapter4rec_amd/_lib.py, whose names this wrapper is also reachable under: raw device pointers, torch's current stream, no
fallback.  _lib.lib() checks and installs the signature table below when it loads the library, beside its own; tests/test_audience_cpu.py holds it
against the header."""
import ctypes as C

import torch

from . import _lib as L

_P, _I = C.c_void_p, C.c_int
AUDIENCE_SIGNATURES = {
    'a4r_topk_users': (_I, (_P,) * 10 + (_I,) * 5),
}


def _table(what, name, t):
    if t.dim() != 2:
        raise ValueError(f'{what}: {name} [rows, E] expected, got {tuple(t.shape)}')
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f'{what}: {name} must be contiguous float32')
    if t.shape[1] not in L.TOPK_E:
        raise ValueError(f'{what}: {name} has E = {t.shape[1]}, supported {L.TOPK_E}')
    if t.data_ptr() & 15:
        raise ValueError(f'{what}: {name} must be 16-byte aligned')
    return t.shape


def topk_users(item_emb, query, user_vec, seen_ptr, seen_idx, elig, k, rows, scores):
    """a4r_topk_users: rows [Q, k] int32 / scores [Q, k] fp32 = the k best rows 1 .. U1-1 of user_vec (fp32 [U1, E], row 0 = a pad row) for each
    query item query[r] (int32 [Q], ids of item_emb rows; item_emb fp32 [N1, E]) by <item_emb[q], user_vec[row]>, the bits of topk_items.  A row is
    never listed for a query whose id is in the row's own seen list seen_idx[seen_ptr[row] .. seen_ptr[row + 1]) (seen_ptr int64 [U1 + 1],
    non-decreasing and inside seen_idx; seen_idx int32, ascending within a row, of any length), nor when elig[row] == 0 (elig uint8 / bool [U1],
    optional).  Score descending, ties by smaller row; short lists end in row 0 / -inf; a query id outside 1 .. N1-1 gets pads only
    (include/a4r_audience.h).  The workspace is allocated here, as topk_similar allocates it."""
    L.require_gpu(item_emb, query, user_vec, seen_ptr, seen_idx, elig, rows, scores)
    what = 'topk_users'
    N1, E = _table(what, 'item_emb', item_emb)
    U1, Eu = _table(what, 'user_vec', user_vec)
    if Eu != E:
        raise ValueError(f'{what}: item_emb [N1, E] and user_vec [U1, E] expected, got {tuple(item_emb.shape)} and {tuple(user_vec.shape)}')
    if query.dim() != 1 or query.dtype != torch.int32 or not query.is_contiguous():
        raise ValueError(f'{what}: query must be contiguous int32 [Q], got {query.dtype} {tuple(query.shape)}')
    Q = query.numel()
    k = L._topk_k(what, k)
    if Q < 1 or N1 < 2 or U1 < 2:
        raise ValueError(f'{what}: Q = {Q} queries, N1 = {N1} item rows and U1 = {U1} user rows (row 0 = the pad row of each): need Q >= 1, N1 >= 2, U1 >= 2')
    if seen_ptr.dtype != torch.int64 or not seen_ptr.is_contiguous() or tuple(seen_ptr.shape) != (U1 + 1,):
        raise ValueError(f'{what}: seen_ptr must be contiguous int64 [U1 + 1 = {U1 + 1}], got {seen_ptr.dtype} {tuple(seen_ptr.shape)}')
    if seen_idx.dim() != 1 or seen_idx.dtype != torch.int32 or not seen_idx.is_contiguous():
        raise ValueError(f'{what}: seen_idx must be contiguous int32 [n], got {seen_idx.dtype} {tuple(seen_idx.shape)}')
    if seen_ptr.data_ptr() & 7:
        raise ValueError(f'{what}: seen_ptr must be 8-byte aligned')
    if elig is not None:
        if elig.dtype not in (torch.uint8, torch.bool) or not elig.is_contiguous() or tuple(elig.shape) != (U1,):
            raise ValueError(f'{what}: elig must be contiguous uint8 or bool [{U1}], one entry per user row')
        if elig.dtype == torch.bool:
            elig = elig.view(torch.uint8)
    L._topk_outputs(what, Q, k, rows, scores, f32='float32')
    if seen_idx.numel() == 0:                 # (an empty list has no data pointer; the kernel reads no id of it)
        seen_idx = torch.zeros(1, dtype=torch.int32, device=user_vec.device)
    ws = torch.empty(L.topk_ws_bytes(Q, U1, k), dtype=torch.uint8, device=user_vec.device)
    L._check(L.lib().a4r_topk_users(L._stream(), L._p(item_emb), L._p(query), L._p(user_vec), L._p(seen_ptr), L._p(seen_idx), L._p(elig), L._p(rows),
                                    L._p(scores), L._p(ws), Q, N1, U1, E, k), 'a4r_topk_users')
    return rows, scores
