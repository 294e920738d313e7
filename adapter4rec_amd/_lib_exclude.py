"""ctypes binding of top-K recommendation with exclusion lists of any length: the a4r_topk_items_excl export of liba4r_hip.so, declared in
include/a4r_exclude.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names this wrapper is also reachable under: raw
device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table below when it loads the library, beside
its own; tests/test_exclude_cpu.py holds it against the header."""
import ctypes as C

import torch

from . import _lib as L

_P, _I = C.c_void_p, C.c_int
EXCLUDE_SIGNATURES = {
    'a4r_topk_items_excl': (_I, (_P,) * 9 + (_I,) * 4),
}


def topk_items_excl(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores):
    """a4r_topk_items_excl: topk_items (cand None) / topk_items_cand (cand uint8 / bool [N1] on the device) with the users' exclusion lists read
    from global memory: excl_ptr int64 [U + 1] (non-decreasing, inside excl_idx), excl_idx int32, ascending within a user, of any length --
    topk_items' 264-id cap does not apply.  Repeats, id 0 and ids outside 1 .. N1-1 match nothing.  On lists both entries serve, ids and scores
    have topk_items' / topk_items_cand's bits (include/a4r_exclude.h).  The workspace is allocated here, as topk_items allocates it."""
    L.require_gpu(prec, item_emb, excl_ptr, excl_idx, ids, scores)
    what = 'topk_items_excl'
    U, N1, E = L._sweep_operands(what, torch.float32, prec, item_emb)
    if cand is not None:
        cand = L.candidate_mask(cand, N1, what)
    k = L._topk_k(what, k)
    if excl_ptr.dtype != torch.int64 or not excl_ptr.is_contiguous() or tuple(excl_ptr.shape) != (U + 1,):
        raise ValueError(f'{what}: excl_ptr must be contiguous int64 [U + 1 = {U + 1}], got {excl_ptr.dtype} {tuple(excl_ptr.shape)}')
    if excl_idx.dim() != 1 or excl_idx.dtype != torch.int32 or not excl_idx.is_contiguous():
        raise ValueError(f'{what}: excl_idx must be contiguous int32 [n], got {excl_idx.dtype} {tuple(excl_idx.shape)}')
    if excl_ptr.data_ptr() & 7:
        raise ValueError(f'{what}: excl_ptr must be 8-byte aligned')
    L._topk_outputs(what, U, k, ids, scores)
    if excl_idx.numel() == 0:                 # (an empty list has no data pointer; the kernel reads no id of it)
        excl_idx = torch.zeros(1, dtype=torch.int32, device=prec.device)
    ws = torch.empty(L.topk_ws_bytes(U, N1, k), dtype=torch.uint8, device=prec.device)
    L._check(L.lib().a4r_topk_items_excl(L._stream(), L._p(prec), L._p(item_emb), L._p(excl_ptr), L._p(excl_idx), L._p(cand), L._p(ids),
                                         L._p(scores), L._p(ws), U, N1, E, k), 'a4r_topk_items_excl')
    return ids, scores
