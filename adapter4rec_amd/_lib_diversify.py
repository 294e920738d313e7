"""ctypes binding of the diversified re-ranking of a top-K list: the a4r_mmr_rerank export of liba4r_hip.so, declared in include/a4r_diversify.h
(which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names this wrapper is also reachable under: raw device pointers,
torch's current stream, no fallback.  _lib.lib() checks and installs the signature table below when it loads the library, beside its own;
tests/test_mmr_cpu.py holds it against the header."""
import ctypes as C
import math

import torch

from . import _lib as L

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
DIVERSIFY_SIGNATURES = {
    'a4r_mmr_rerank': (_I, (_P,) * 7 + (_F,) + (_I,) * 5),
}
MMR_MAX_POOL = 256         # A4R_MMR_MAX_POOL (include/a4r_diversify.h) = TOPK_MAX_K: the pool is a top-K output


def mmr_rerank(item_emb, pool_ids, pool_scores, lam, k, ids, scores, ild=None):
    """a4r_mmr_rerank: ids [U, k] int32 / scores [U, k] fp32 = k entries of each user's pool (pool_ids int32 / pool_scores fp32 [U, P], P at most
    MMR_MAX_POOL: a top-K output with K = P) picked greedily by lam * relevance - (1 - lam) * (largest cosine to an entry already picked), ties to
    the smaller pool position; the scores are the pool's own, in pick order.  ild (fp32 [U], optional): the mean of 1 - cosine over the pairs of
    picked entries.  The rule: include/a4r_diversify.h.  One launch, no workspace."""
    L.require_gpu(item_emb, pool_ids, pool_scores, ids, scores, ild)
    what = 'mmr_rerank'
    k, lam = int(k), float(lam)
    if item_emb.dim() != 2 or pool_ids.dim() != 2 or tuple(pool_scores.shape) != tuple(pool_ids.shape):
        raise ValueError(f'{what}: item_emb [N1, E] and pool_ids / pool_scores [U, P] expected, got {tuple(item_emb.shape)}, {tuple(pool_ids.shape)} '
                         f'and {tuple(pool_scores.shape)}')
    N1, E = item_emb.shape
    U, P = pool_ids.shape
    for name, t, dt in (('item_emb', item_emb, torch.float32), ('pool_ids', pool_ids, torch.int32), ('pool_scores', pool_scores, torch.float32),
                        ('ids', ids, torch.int32), ('scores', scores, torch.float32), ('ild', ild, torch.float32)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise ValueError(f'{what}: {name} must be contiguous {str(dt).replace("torch.", "")}')
    if E not in L.TOPK_E:
        raise ValueError(f'{what}: E = {E}, supported {L.TOPK_E}')
    if U < 1 or N1 < 2:
        raise ValueError(f'{what}: U = {U} users and N1 = {N1} table rows (row 0 = the pad item): need U >= 1, N1 >= 2')
    if item_emb.data_ptr() & 15:
        raise ValueError(f'{what}: item_emb must be 16-byte aligned')
    if not 1 <= P <= MMR_MAX_POOL:
        raise ValueError(f'{what}: pool of P = {P} entries outside 1 .. {MMR_MAX_POOL}')
    if not 1 <= k <= P:
        raise ValueError(f'{what}: k = {k} outside 1 .. P = {P}')
    if math.isnan(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f'{what}: lambda = {lam} outside [0, 1]')
    if tuple(ids.shape) != (U, k) or tuple(scores.shape) != (U, k):
        raise ValueError(f'{what}: ids and scores must be [{U}, {k}]')
    if ild is not None and tuple(ild.shape) != (U,):
        raise ValueError(f'{what}: ild must be [{U}], got {tuple(ild.shape)}')
    L._check(L.lib().a4r_mmr_rerank(L._stream(), L._p(item_emb), L._p(pool_ids), L._p(pool_scores), L._p(ids), L._p(scores), L._p(ild), lam, U, N1, E,
                                    P, k), 'a4r_mmr_rerank')
    return ids, scores
