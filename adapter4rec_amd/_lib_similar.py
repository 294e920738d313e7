"""ctypes binding of the similar-item queries: the a4r_row_inv_norms / a4r_topk_similar exports of liba4r_hip.so, declared in
include/a4r_similar.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names these wrappers are also reachable under:
raw device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table below when it loads the library,
beside its own; tests/test_similar_cpu.py holds it against the header prototype by prototype."""
import ctypes as C
import math

import torch

from . import _lib as L

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
SIMILAR_SIGNATURES = {
    'a4r_row_inv_norms': (_I, (_P, _P, _P, _I, _I)),
    'a4r_topk_similar': (_I, (_P,) * 5 + (_F,) + (_P,) * 3 + (_I,) * 4),
}


def _table(what, item_emb):
    if item_emb.dim() != 2:
        raise ValueError(f'{what}: item_emb [N1, E] expected, got {tuple(item_emb.shape)}')
    N1, E = item_emb.shape
    if item_emb.dtype != torch.float32 or not item_emb.is_contiguous():
        raise ValueError(f'{what}: item_emb must be contiguous float32')
    if E not in L.TOPK_E:
        raise ValueError(f'{what}: E = {E}, supported {L.TOPK_E}')
    if item_emb.data_ptr() & 15:
        raise ValueError(f'{what}: item_emb must be 16-byte aligned')
    return N1, E


def row_inv_norms(table, out=None):
    """a4r_row_inv_norms: out fp32 [N1] (allocated here when None) = 1 / the Euclidean norm of every row of table (fp32 [N1, E]), the squares summed
    in fp64 and the result rounded to fp32 once; 0 for a zero row and for a row holding inf or NaN (include/a4r_similar.h).  One launch."""
    L.require_gpu(table, out)
    what = 'row_inv_norms'
    N1, E = _table(what, table)
    if N1 < 1:
        raise ValueError(f'{what}: N1 = {N1} table rows: need N1 >= 1')
    if out is None:
        out = torch.empty(N1, dtype=torch.float32, device=table.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (N1,):
        raise ValueError(f'{what}: out must be contiguous float32 [{N1}]')
    L._check(L.lib().a4r_row_inv_norms(L._stream(), L._p(table), L._p(out), N1, E), 'a4r_row_inv_norms')
    return out


def topk_similar(item_emb, inv_norm, query, cand, min_sim, k, ids, scores):
    """a4r_topk_similar: ids [Q, k] int32 / scores [Q, k] fp32 = the k nearest other items 1 .. N1-1 of each query item query[r] (int32 [Q]).
    inv_norm (row_inv_norms' output, fp32 [N1]): cosine, score = dot * (inv_norm[q] * inv_norm[i]); None: the dot product, the bits of
    topk_items.  cand (uint8 / bool [N1], optional): neighbours come from the items with cand[i] != 0.  min_sim (None or -inf: no floor): items
    scoring below it are not listed.  Score descending, ties by smaller id; short lists end in id 0 / -inf; a query id outside 1 .. N1-1, or (cosine)
    a query with a zero or non-finite row, gets pads only (include/a4r_similar.h).  The workspace is allocated here, as topk_items allocates it."""
    L.require_gpu(item_emb, inv_norm, query, cand, ids, scores)
    what = 'topk_similar'
    min_sim = -math.inf if min_sim is None else float(min_sim)
    N1, E = _table(what, item_emb)
    if query.dim() != 1 or query.dtype != torch.int32 or not query.is_contiguous():
        raise ValueError(f'{what}: query must be contiguous int32 [Q], got {query.dtype} {tuple(query.shape)}')
    Q = query.numel()
    k = L._topk_k(what, k)
    if Q < 1 or N1 < 2:
        raise ValueError(f'{what}: Q = {Q} queries and N1 = {N1} table rows (row 0 = the pad item): need Q >= 1, N1 >= 2')
    if inv_norm is not None and (inv_norm.dtype != torch.float32 or not inv_norm.is_contiguous() or tuple(inv_norm.shape) != (N1,)):
        raise ValueError(f'{what}: inv_norm must be contiguous float32 [{N1}]')
    if cand is not None:
        if cand.dtype not in (torch.uint8, torch.bool) or not cand.is_contiguous() or tuple(cand.shape) != (N1,):
            raise ValueError(f'{what}: cand must be contiguous uint8 or bool [{N1}], one entry per table row')
        if cand.dtype == torch.bool:
            cand = cand.view(torch.uint8)
    if math.isnan(min_sim):
        raise ValueError(f'{what}: min_sim is NaN')
    L._topk_outputs(what, Q, k, ids, scores, f32='float32')
    ws = torch.empty(L.topk_ws_bytes(Q, N1, k), dtype=torch.uint8, device=item_emb.device)
    L._check(L.lib().a4r_topk_similar(L._stream(), L._p(item_emb), L._p(inv_norm), L._p(query), L._p(cand), min_sim, L._p(ids), L._p(scores), L._p(ws),
                                      Q, N1, E, k), 'a4r_topk_similar')
    return ids, scores
