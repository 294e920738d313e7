"""ctypes binding of evaluation and top-K recommendation with scores from the bf16 MFMA (--score_dtype bf16): the a4r_eval_rank_bf16 /
a4r_topk_items_bf16 / a4r_topk_bf16_ws_bytes exports of liba4r_hip.so, declared in include/a4r_score_bf16.h (which include/a4r.h includes).  Same
rules as adapter4rec_amd/_lib.py, whose names these wrappers are also reachable under: raw device pointers, torch's current stream, no fallback.
_lib.lib() checks and installs the signature table below when it loads the library, beside its own; tests/test_score_bf16_cpu.py holds it against
the header prototype by prototype.  The operands are the bf16 copies _lib_ce_bf16.cast_bf16 writes: there is no second cast."""
import ctypes as C

import torch

from . import _lib as L
from ._lib_candidates import candidate_mask

_P, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SCORE_BF16_SIGNATURES = {
    'a4r_topk_bf16_ws_bytes': (_SZ, (_I, _I, _I, _I)),
    'a4r_eval_rank_bf16': (_I, (_P,) * 8 + (_I,) * 3),
    'a4r_topk_items_bf16': (_I, (_P,) * 9 + (_I,) * 4),
}


def topk_bf16_ws_bytes(U, N1, E, k):
    """Bytes of a4r_topk_items_bf16's workspace (a host-side query, no GPU); 0 for a shape the kernel refuses.  It depends on E: the bf16 kernels
    hold 16 or 32 users a workgroup depending on E and k, and the grid follows."""
    return int(L.lib().a4r_topk_bf16_ws_bytes(U, N1, E, k))


def eval_rank_bf16(prec_b, table_b, target, hist_ptr, hist_idx, rank, cand=None):
    """a4r_eval_rank_bf16: eval_rank (cand None) or eval_rank_cand (cand uint8 / bool [N1] on the device) with score(u, i) = <prec_b[u], table_b[i]>
    from the bf16 MFMA, accumulated in fp32 (include/a4r_score_bf16.h).  prec_b [U, E], table_b [N1, E]: contiguous bf16."""
    L.require_gpu(prec_b, table_b, target, hist_ptr, hist_idx, rank)
    U, N1, E = L._sweep_operands('eval_rank_bf16', torch.bfloat16, prec_b, table_b)
    if cand is not None:
        cand = candidate_mask(cand, N1, 'eval_rank_bf16')
    for name, t, n in (('target', target, U), ('hist_ptr', hist_ptr, U + 1), ('hist_idx', hist_idx, 1), ('rank', rank, U)):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f'eval_rank_bf16: {name} must be contiguous int32 of at least {n} elements')
    L._check(L.lib().a4r_eval_rank_bf16(L._stream(), L._p(prec_b), L._p(table_b), L._p(target), L._p(hist_ptr), L._p(hist_idx), L._p(cand), L._p(rank),
                                        U, N1, E), 'a4r_eval_rank_bf16')


def topk_items_bf16(prec_b, table_b, excl_ptr, excl_idx, k, ids, scores, cand=None):
    """a4r_topk_items_bf16: topk_items (cand None) or topk_items_cand (cand uint8 / bool [N1] on the device) with the scores of eval_rank_bf16 --
    the same bits.  Everything else, the argument checks and the workspace allocated here included, as topk_items."""
    L.require_gpu(prec_b, table_b, excl_ptr, excl_idx, ids, scores)
    U, N1, E = L._sweep_operands('topk_items_bf16', torch.bfloat16, prec_b, table_b)
    if cand is not None:
        cand = candidate_mask(cand, N1, 'topk_items_bf16')
    k, excl_idx, ws = L._topk_args('topk_items_bf16', prec_b.device, U, excl_ptr, excl_idx, k, ids, scores, lambda k: topk_bf16_ws_bytes(U, N1, E, k))
    L._check(L.lib().a4r_topk_items_bf16(L._stream(), L._p(prec_b), L._p(table_b), L._p(excl_ptr), L._p(excl_idx), L._p(cand), L._p(ids), L._p(scores),
                                         L._p(ws), U, N1, E, k), 'a4r_topk_items_bf16')
    return ids, scores
