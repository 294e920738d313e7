"""ctypes binding of top-K recommendation and evaluation within a candidate list of each user's own: the a4r_topk_lists / a4r_eval_rank_lists exports
of liba4r_hip.so, declared in include/a4r_user_lists.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names these
wrappers are also reachable under: raw device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table
below when it loads the library, beside its own; tests/test_user_lists_cpu.py holds it against the header prototype by prototype."""
import ctypes as C

import torch

from . import _lib as L

_P, _I = C.c_void_p, C.c_int
USER_LISTS_SIGNATURES = {
    'a4r_topk_lists': (_I, (_P,) * 9 + (_I,) * 5),
    'a4r_eval_rank_lists': (_I, (_P,) * 9 + (_I,) * 4),
}
LIST_MAX = 4096            # A4R_LIST_MAX (include/a4r_user_lists.h)


def _check_common(what, prec, item_emb, list_ptr, list_idx, max_len, x_name, x_ptr, x_idx):
    """The checks both wrappers share -> (U, N1, E, max_len, list_idx, x_idx), the two id tensors replaced by a one-element zero tensor where
    they are empty (an empty tensor has no data pointer; the kernel reads no id of it)."""
    if prec.dim() != 2 or item_emb.dim() != 2 or prec.shape[1] != item_emb.shape[1]:
        raise ValueError(f'{what}: prec [U, E] and item_emb [N1, E] expected, got {tuple(prec.shape)} and {tuple(item_emb.shape)}')
    U, E = prec.shape
    N1 = item_emb.shape[0]
    for name, t in (('prec', prec), ('item_emb', item_emb)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous fp32')
    if E not in L.TOPK_E:
        raise ValueError(f'{what}: E = {E}, supported {L.TOPK_E}')
    if U < 1 or N1 < 2:
        raise ValueError(f'{what}: U = {U} users and N1 = {N1} table rows (row 0 = the pad item): need U >= 1, N1 >= 2')
    for name, t in (('prec', prec), ('item_emb', item_emb)):
        if t.data_ptr() & 15:
            raise ValueError(f'{what}: {name} must be 16-byte aligned')
    max_len = int(max_len)
    if not 0 <= max_len <= LIST_MAX:
        raise ValueError(f'{what}: max_len = {max_len} outside 0 .. {LIST_MAX}')
    for name, t in (('list_ptr', list_ptr), ('list_idx', list_idx), (x_name + '_ptr', x_ptr), (x_name + '_idx', x_idx)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous int32')
    for name, t in (('list_ptr', list_ptr), (x_name + '_ptr', x_ptr)):
        if t.dim() != 1 or t.numel() != U + 1:
            raise ValueError(f'{what}: {name} must hold U + 1 = {U + 1} offsets, got {tuple(t.shape)}')
    if list_idx.numel() == 0:
        list_idx = torch.zeros(1, dtype=torch.int32, device=prec.device)
    if x_idx.numel() == 0:
        x_idx = torch.zeros(1, dtype=torch.int32, device=prec.device)
    return U, N1, E, max_len, list_idx, x_idx


def topk_lists(prec, item_emb, list_ptr, list_idx, max_len, excl_ptr, excl_idx, k, ids, scores):
    """a4r_topk_lists: ids [U, k] int32 / scores [U, k] fp32 = the k best distinct items of the user's own list
    list_idx[list_ptr[u] .. list_ptr[u + 1]) (its first ``max_len`` entries: the caller, who built the CSR on the host, passes the longest length,
    at most LIST_MAX; nothing is read back from the device to find it) outside the user's exclusion list; order, ties and pad slots as topk_items
    (include/a4r_user_lists.h).  One launch, no workspace."""
    L.require_gpu(prec, item_emb, list_ptr, list_idx, excl_ptr, excl_idx, ids, scores)
    what = 'topk_lists'
    k = int(k)
    U, N1, E, max_len, list_idx, excl_idx = _check_common(what, prec, item_emb, list_ptr, list_idx, max_len, 'excl', excl_ptr, excl_idx)
    if not 1 <= k <= L.TOPK_MAX_K:
        raise ValueError(f'{what}: k = {k} outside 1 .. {L.TOPK_MAX_K}')
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError(f'{what}: ids must be contiguous int32')
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError(f'{what}: scores must be contiguous fp32')
    if tuple(ids.shape) != (U, k) or tuple(scores.shape) != (U, k):
        raise ValueError(f'{what}: ids and scores must be [{U}, {k}]')
    L._check(L.lib().a4r_topk_lists(L._stream(), L._p(prec), L._p(item_emb), L._p(list_ptr), L._p(list_idx), L._p(excl_ptr), L._p(excl_idx), L._p(ids),
                                    L._p(scores), U, N1, E, k, max_len), 'a4r_topk_lists')
    return ids, scores


def eval_rank_lists(prec, item_emb, target, list_ptr, list_idx, max_len, hist_ptr, hist_idx, rank):
    """a4r_eval_rank_lists: rank [U] int32 = 1 + the distinct items of the user's own list, outside the user's history, that score above
    target[u]; the target need not be listed (include/a4r_user_lists.h).  Lists and ``max_len`` as topk_lists."""
    L.require_gpu(prec, item_emb, target, list_ptr, list_idx, hist_ptr, hist_idx, rank)
    what = 'eval_rank_lists'
    U, N1, E, max_len, list_idx, hist_idx = _check_common(what, prec, item_emb, list_ptr, list_idx, max_len, 'hist', hist_ptr, hist_idx)
    for name, t in (('target', target), ('rank', rank)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous int32')
        if t.dim() != 1 or t.numel() != U:
            raise ValueError(f'{what}: {name} must be [{U}], got {tuple(t.shape)}')
    L._check(L.lib().a4r_eval_rank_lists(L._stream(), L._p(prec), L._p(item_emb), L._p(target), L._p(list_ptr), L._p(list_idx), L._p(hist_ptr),
                                         L._p(hist_idx), L._p(rank), U, N1, E, max_len), 'a4r_eval_rank_lists')
    return rank
