"""ctypes binding of the sampled evaluation's negatives drawn on the device: the a4r_eval_draw_negatives / a4r_eval_rank_sampled exports of
liba4r_hip.so, declared in include/a4r_eval_negatives.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names these
wrappers are also reachable under: raw device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table
below when it loads the library, beside its own; tests/test_eval_negatives_cpu.py holds it against the header prototype by prototype."""
import ctypes as C

import torch

from . import _lib as L
from ._lib_user_lists import LIST_MAX

_P, _I, _U64 = C.c_void_p, C.c_int, C.c_uint64
EVAL_NEGATIVES_SIGNATURES = {
    'a4r_eval_draw_negatives': (_I, (_P,) * 6 + (_U64,) + (_P,) * 2 + (_I,) * 3),
    'a4r_eval_rank_sampled': (_I, (_P,) * 8 + (_U64,) + (_P,) * 2 + (_I,) * 4),
}
EVAL_NEG_SITE = 7002       # A4R_EVAL_NEG_SITE (include/a4r_eval_negatives.h): the hash site of the draws
EVAL_NEG_MAX = LIST_MAX    # N <= A4R_LIST_MAX


def _check_draw(what, target, hist_ptr, hist_idx, user_key, cdf, seed, n, err, N1):
    """The checks both wrappers share -> (U, n, seed, hist_idx), an empty hist_idx replaced by a one-element zero tensor (an empty tensor has no
    data pointer; the kernel reads no id of it)."""
    for name, t in (('target', target), ('hist_ptr', hist_ptr), ('hist_idx', hist_idx), ('user_key', user_key), ('err', err)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous int32')
    if target.dim() != 1 or target.numel() < 1:
        raise ValueError(f'{what}: target must be [U] with U >= 1, got {tuple(target.shape)}')
    U = target.numel()
    if N1 < 2:
        raise ValueError(f'{what}: N1 = {N1} table rows (row 0 = the pad item): need N1 >= 2')
    if hist_ptr.dim() != 1 or hist_ptr.numel() != U + 1:
        raise ValueError(f'{what}: hist_ptr must hold U + 1 = {U + 1} offsets, got {tuple(hist_ptr.shape)}')
    if user_key.dim() != 1 or user_key.numel() != U:
        raise ValueError(f'{what}: user_key must be [{U}], got {tuple(user_key.shape)}')
    if err.numel() != 1:
        raise ValueError(f'{what}: err must hold one int32, got {tuple(err.shape)}')
    if cdf is not None:
        if cdf.dtype != torch.int64 or not cdf.is_contiguous():
            raise ValueError(f'{what}: cdf must be contiguous int64')
        if cdf.dim() != 1 or cdf.numel() != N1:
            raise ValueError(f'{what}: cdf must be [{N1}] (cdf[0] = 0, one entry per table row), got {tuple(cdf.shape)}')
    n = int(n)
    if not 1 <= n <= EVAL_NEG_MAX:
        raise ValueError(f'{what}: n = {n} negatives outside 1 .. {EVAL_NEG_MAX}')
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f'{what}: seed = {seed} outside 0 .. 2^64 - 1')
    if hist_idx.numel() == 0:
        hist_idx = torch.zeros(1, dtype=torch.int32, device=target.device)
    return U, n, seed, hist_idx


def eval_draw_negatives(hist_ptr, hist_idx, target, user_key, cdf, seed, n1, out_ids, err):
    """a4r_eval_draw_negatives: out_ids [U, n] int32 = the n negatives of every user's sampled evaluation by the rule of
    include/a4r_eval_negatives.h: a pure function of (seed, user_key[u], j, the user's history and target, cdf).  ``cdf``: None = uniform, or
    int64 [n1] cumulative occurrence counts (popularity sampling).  ``err`` int32 [1] is added to (one per user without a candidate), never
    cleared.  One launch, no workspace."""
    L.require_gpu(hist_ptr, hist_idx, target, user_key, cdf, out_ids, err)
    what = 'eval_draw_negatives'
    n1 = int(n1)
    if out_ids.dim() != 2:
        raise ValueError(f'{what}: out_ids must be [U, n], got {tuple(out_ids.shape)}')
    U, n, seed, hist_idx = _check_draw(what, target, hist_ptr, hist_idx, user_key, cdf, seed, out_ids.shape[1], err, n1)
    if out_ids.dtype != torch.int32 or not out_ids.is_contiguous() or tuple(out_ids.shape) != (U, n):
        raise ValueError(f'{what}: out_ids must be contiguous int32 [{U}, {n}]')
    L._check(L.lib().a4r_eval_draw_negatives(L._stream(), L._p(hist_ptr), L._p(hist_idx), L._p(target), L._p(user_key), L._p(cdf), seed,
                                             L._p(out_ids), L._p(err), U, n1, n), 'a4r_eval_draw_negatives')
    return out_ids


def eval_rank_sampled(prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, seed, n, rank, err):
    """a4r_eval_rank_sampled: rank [U] int32 = 1 + the distinct items among the user's n drawn negatives (eval_draw_negatives' draws, never
    written to memory) that score above target[u]; scores and comparison as eval_rank_lists'.  One launch, no workspace."""
    L.require_gpu(prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, rank, err)
    what = 'eval_rank_sampled'
    if prec.dim() != 2 or item_emb.dim() != 2 or prec.shape[1] != item_emb.shape[1]:
        raise ValueError(f'{what}: prec [U, E] and item_emb [N1, E] expected, got {tuple(prec.shape)} and {tuple(item_emb.shape)}')
    E = prec.shape[1]
    N1 = item_emb.shape[0]
    for name, t in (('prec', prec), ('item_emb', item_emb)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous fp32')
    if E not in L.TOPK_E:
        raise ValueError(f'{what}: E = {E}, supported {L.TOPK_E}')
    for name, t in (('prec', prec), ('item_emb', item_emb)):
        if t.data_ptr() & 15:
            raise ValueError(f'{what}: {name} must be 16-byte aligned')
    U, n, seed, hist_idx = _check_draw(what, target, hist_ptr, hist_idx, user_key, cdf, seed, n, err, N1)
    if prec.shape[0] != U:
        raise ValueError(f'{what}: prec has {prec.shape[0]} rows, target {U}')
    if rank.dtype != torch.int32 or not rank.is_contiguous() or rank.dim() != 1 or rank.numel() != U:
        raise ValueError(f'{what}: rank must be contiguous int32 [{U}], got {tuple(rank.shape)}')
    L._check(L.lib().a4r_eval_rank_sampled(L._stream(), L._p(prec), L._p(item_emb), L._p(target), L._p(hist_ptr), L._p(hist_idx), L._p(user_key),
                                           L._p(cdf), seed, L._p(rank), L._p(err), U, N1, E, n), 'a4r_eval_rank_sampled')
    return rank
