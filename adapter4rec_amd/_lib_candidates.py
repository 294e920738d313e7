"""ctypes binding of evaluation and top-K recommendation within a candidate set of items: the a4r_eval_rank_cand / a4r_topk_items_cand exports of
liba4r_hip.so, declared in include/a4r_candidates.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names these
wrappers are also reachable under: raw device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table
below when it loads the library, beside its own; tests/test_candidates_cpu.py holds it against the header prototype by prototype."""
import ctypes as C

import torch

from . import _lib as L

_P, _I = C.c_void_p, C.c_int
CANDIDATES_SIGNATURES = {
    'a4r_eval_rank_cand': (_I, (_P,) * 8 + (_I,) * 3),
    'a4r_topk_items_cand': (_I, (_P,) * 9 + (_I,) * 4),
}


def candidate_mask(cand, N1, what):
    """The candidate set as the kernels read it: a contiguous uint8 device tensor of N1 bytes (a torch.bool tensor is one as it stands: viewed,
    not copied).  Anything else raises ValueError."""
    if not isinstance(cand, torch.Tensor):
        raise ValueError(f'{what}: cand must be a uint8 or bool tensor of N1 = {N1} elements, got {type(cand).__name__}')
    if cand.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f'{what}: cand must be uint8 or bool, got {cand.dtype}')
    if cand.dim() != 1 or cand.numel() != N1:
        raise ValueError(f'{what}: cand must hold one entry per table row, [{N1}], got {tuple(cand.shape)}')
    if not cand.is_contiguous():
        raise ValueError(f'{what}: cand must be contiguous')
    if not cand.is_cuda:
        raise ValueError(f'{what}: cand must be a device tensor (the kernels read it from device memory)')
    return cand.view(torch.uint8) if cand.dtype == torch.bool else cand


def eval_rank_cand(prec, item_emb, target, hist_ptr, hist_idx, cand, rank):
    """a4r_eval_rank_cand: eval_rank counting only the items i with cand[i] != 0 (uint8 / bool [N1] on the device, cand[0] ignored).  The target
    need not be a candidate: its rank is then the one it would have if it were (include/a4r_candidates.h)."""
    L.require_gpu(prec, item_emb, target, hist_ptr, hist_idx, rank)
    cand = candidate_mask(cand, item_emb.shape[0], 'eval_rank_cand')
    L._check(L.lib().a4r_eval_rank_cand(L._stream(), L._p(prec), L._p(item_emb), L._p(target), L._p(hist_ptr), L._p(hist_idx), L._p(cand), L._p(rank),
                                        prec.shape[0], item_emb.shape[0], prec.shape[1]), 'a4r_eval_rank_cand')


def topk_items_cand(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores):
    """a4r_topk_items_cand: topk_items over the items i with cand[i] != 0 (uint8 / bool [N1] on the device, cand[0] ignored) that are not in the
    user's exclusion list; everything else, the argument checks and the workspace allocated here included, as topk_items."""
    L.require_gpu(prec, item_emb, excl_ptr, excl_idx, ids, scores)
    U, N1, E = L._sweep_operands('topk_items_cand', torch.float32, prec, item_emb)
    cand = candidate_mask(cand, N1, 'topk_items_cand')
    k, excl_idx, ws = L._topk_args('topk_items_cand', prec.device, U, excl_ptr, excl_idx, k, ids, scores, lambda k: L.topk_ws_bytes(U, N1, k))
    L._check(L.lib().a4r_topk_items_cand(L._stream(), L._p(prec), L._p(item_emb), L._p(excl_ptr), L._p(excl_idx), L._p(cand), L._p(ids), L._p(scores),
                                         L._p(ws), U, N1, E, k), 'a4r_topk_items_cand')
    return ids, scores
