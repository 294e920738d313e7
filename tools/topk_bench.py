#!/usr/bin/env python
"""Top-K recommendation on one MI355X: a4r_topk_items beside a4r_eval_rank (the same scoring sweep, one rank per user) and beside the torch path a
user would otherwise write (chunked fp32 matmul, history masked, torch.topk), and recommend() end to end -- one JSON line per configuration.

    python tools/topk_bench.py [--iters N] [--only NAME] [--candidates FRACTION] [--lists C] [--mmr] [--similar] [--bf16] [--audience] [--exclude]

--exclude runs the exclusion-list leg instead (exclude_cfg): a4r_topk_items_excl for 32 768 users of a 65 537-row table, K = 10 and 100, E = 64 and
128, (a) beside a4r_topk_items of the same build on identical lists of 20 and of 264 ids, (b) at 1 000 and 5 000 ids per user -- drawn uniformly, and
the user's own best items -- beside eager torch (chunked matmul, listed pairs set to -inf, topk), three interleaved rounds after a warm-up (the
numbers land in profiles/exclude_bench.jsonl).

--bf16 runs the bf16-score leg instead (bf16_cfg): a4r_topk_items_bf16 beside a4r_topk_items / a4r_topk_items_cand of the same build, 32 768 users,
65 537 items at E = 64 .. 512 and 500 001 items at E = 64 / 128, K = 10 / 100 / 256, the candidate set off and at 0.1, the casts in one leg and outside
another, interleaved rounds after a warm-up (the numbers land in profiles/score_bf16_bench.jsonl).

--candidates FRACTION runs the candidate-set leg instead (cand_cfg): a4r_topk_items_cand / a4r_eval_rank_cand beside the unmasked entries, interleaved.
--lists C runs the per-user-list leg instead (lists_cfg): a4r_topk_lists over C listed items per user (C = 0: 100, 1000 and 4096 in turn), E = 64 and
128, beside the eager path a caller without the kernel writes (chunked emb[idx] gather, einsum, exclusion mask, torch.topk), interleaved, and beside
a4r_topk_items over the whole table for scale.
--mmr runs the re-ranking leg instead (mmr_cfg): a4r_mmr_rerank cutting a4r_topk_items' pools of 100 and 256 items to 10, E = 64 and 128, lambda 0.7,
beside the eager composition on the same pools (gather, bmm cosine matrix, a K-round loop from the host), interleaved.
--similar runs the similar-items leg instead (similar_cfg): a4r_topk_similar (cosine) for 32 768 query items of a 65 537-row table, K = 10 and 100,
E = 64 and 128, beside the composition of existing entries (normalised copy + gather + a4r_topk_items with one-id exclusion lists) and beside eager
torch (normalise, chunked matmul, topk), interleaved rounds after a warm-up.
--audience runs the audience leg instead (audience_cfg): a4r_topk_users for 4 096 query items over a user table of 262 145 rows, 20 seen ids per user,
K = 10 and 100, E = 64 and 128, beside the role-swapped a4r_topk_items with empty exclusion lists (the nearest existing launch: it answers another
question, no user is left out) and beside eager torch (chunked matmul, seen pairs set to -inf, topk), three interleaved rounds after a warm-up (the
numbers land in profiles/audience_bench.jsonl).

Shapes: 32 768 users x 65 537 items (the evaluation benchmark's shape) and x 500 001 items (the ID tower's 500 000-item table), E = 64, K 10 / 100,
histories of 20 uniform ids.  Kernel times are HIP-event means over N launches after a warm-up; per-kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/topk_bench.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def data(U, N1, E, H, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    emb = torch.randn(N1, E, device=DEV, generator=g)
    prec = torch.randn(U, E, device=DEV, generator=g)
    hist = torch.randint(1, N1, (U, H), device=DEV, generator=g, dtype=torch.int32)
    ptr = (torch.arange(U + 1, device=DEV, dtype=torch.int32) * H).contiguous()
    tgt = torch.randint(1, N1, (U,), device=DEV, generator=g, dtype=torch.int32)
    return emb, prec, hist, ptr, tgt


def torch_path(prec, emb, hist, k, chunk=2048):
    """what a caller without the kernel writes: [chunk, N1] fp32 scores, pad + history masked, torch.topk"""
    ids, scores = [], []
    for a in range(0, prec.shape[0], chunk):
        s = prec[a:a + chunk] @ emb.t()
        s[:, 0] = -float('inf')
        s.scatter_(1, hist[a:a + chunk].long(), -float('inf'))
        v, i = torch.topk(s, k, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def kernel_cfg(name, U, N1, E, k, iters, H=20):
    from adapter4rec_amd import _lib as L
    emb, prec, hist, ptr, tgt = data(U, N1, E, H)
    flat = hist.reshape(-1).contiguous()
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    rank = torch.zeros(U, dtype=torch.int32, device=DEV)
    t_topk = timed(lambda: L.topk_items(prec, emb, ptr, flat, k, ids, sc), iters)
    t_eval = timed(lambda: L.eval_rank(prec, emb, tgt, ptr, flat, rank), iters)
    t_torch = timed(lambda: torch_path(prec, emb, hist, k), max(1, iters // 4))
    ti, ts = torch_path(prec, emb, hist, k)
    agree = float((ti.int() == ids).float().mean())                 # random fp32 data: the lists agree up to near-ties
    return dict(name=name, users=U, items=N1, E=E, k=k, topk_ms=round(t_topk, 4), eval_rank_ms=round(t_eval, 4), torch_ms=round(t_torch, 3),
                topk_over_eval=round(t_topk / t_eval, 3), torch_over_topk=round(t_torch / t_topk, 2), users_per_s=round(U / t_topk * 1e3),
                id_agreement_with_torch=round(agree, 6))


def cand_cfg(name, U, N1, E, k, fraction, iters, rounds=2, H=20):
    """--candidates FRACTION: a4r_topk_items_cand and a4r_eval_rank_cand under a random candidate set of that fraction of the items (1.0: every
    item) beside the unmasked entries on the same data, the four legs interleaved `rounds` times; every round's mean is reported."""
    from adapter4rec_amd import _lib as L
    emb, prec, hist, ptr, tgt = data(U, N1, E, H)
    flat = hist.reshape(-1).contiguous()
    g = torch.Generator(device=DEV).manual_seed(1)
    cand = (torch.rand(N1, device=DEV, generator=g) < fraction).to(torch.uint8).contiguous()
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    rank = torch.zeros(U, dtype=torch.int32, device=DEV)
    legs = dict(topk=lambda: L.topk_items(prec, emb, ptr, flat, k, ids, sc), topk_cand=lambda: L.topk_items_cand(prec, emb, ptr, flat, cand, k, ids, sc),
                eval_rank=lambda: L.eval_rank(prec, emb, tgt, ptr, flat, rank), eval_rank_cand=lambda: L.eval_rank_cand(prec, emb, tgt, ptr, flat, cand, rank))
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters), 4))
    return dict(name=name, users=U, items=N1, E=E, k=k, fraction=fraction, candidates=int(cand[1:].ne(0).sum()), rounds=rounds, iters=iters,
                **{n + '_ms': v for n, v in ms.items()}, topk_cand_over_topk=round(min(ms['topk_cand']) / min(ms['topk']), 3),
                eval_rank_cand_over_eval_rank=round(min(ms['eval_rank_cand']) / min(ms['eval_rank']), 3))


def eager_lists(prec, emb, idx, hist, k, chunk):
    """what a caller without the kernel writes: gather the listed rows of a chunk of users, one dot product per row, the user's history masked,
    torch.topk, the ids looked up (the lists here hold distinct items, so nothing has to be deduplicated)"""
    ids, scores = [], []
    for a in range(0, prec.shape[0], chunk):
        ix = idx[a:a + chunk].long()
        s = torch.einsum('uce,ue->uc', emb[ix], prec[a:a + chunk])
        s.masked_fill_((ix[:, :, None] == hist[a:a + chunk].long()[:, None, :]).any(-1), -float('inf'))
        v, i = torch.topk(s, k, dim=1)
        ids.append(torch.gather(ix, 1, i))
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def lists_cfg(name, U, N1, E, k, C, iters, rounds=2, H=20):
    """--lists C: every user lists C distinct items (a random start and an odd stride through the N1 - 1 = 2^16 items); a4r_topk_lists and the
    eager path interleaved `rounds` times, every round's mean reported; a4r_topk_items over the whole table once, for scale.  gather_GBps: the
    listed rows' bytes, U * C * E * 4, over the kernel's best time."""
    from adapter4rec_amd import _lib as L
    assert (N1 - 1) & (N1 - 2) == 0 and C <= N1 - 1
    emb, prec, hist, ptr, tgt = data(U, N1, E, H)
    flat = hist.reshape(-1).contiguous()
    g = torch.Generator(device=DEV).manual_seed(2)
    start = torch.randint(0, N1 - 1, (U, 1), device=DEV, generator=g)
    stride = torch.randint(0, (N1 - 1) // 2, (U, 1), device=DEV, generator=g) * 2 + 1
    idx = ((start + stride * torch.arange(C, device=DEV)[None]) % (N1 - 1) + 1).to(torch.int32).contiguous()
    lptr = (torch.arange(U + 1, device=DEV, dtype=torch.int32) * C).contiguous()
    lflat = idx.reshape(-1)
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    chunk = max(1, (1 << 28) // (C * E))                            # 1 GiB of gathered rows per chunk
    legs = dict(topk_lists=lambda: L.topk_lists(prec, emb, lptr, lflat, C, ptr, flat, k, ids, sc), eager=lambda: eager_lists(prec, emb, idx, hist, k, chunk))
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters if n == 'topk_lists' else max(1, iters // 4)), 4))
    ei, _ = eager_lists(prec, emb, idx, hist, k, chunk)
    legs['topk_lists']()
    agree = float((ei.int() == ids).float().mean())                 # random fp32 data: the lists agree up to near-ties
    ids_t = torch.empty(U, k, dtype=torch.int32, device=DEV)
    t_table = timed(lambda: L.topk_items(prec, emb, ptr, flat, k, ids_t, sc), max(1, iters // 4))
    best = min(ms['topk_lists'])
    return dict(name=name, users=U, items=N1, E=E, k=k, listed=C, rounds=rounds, iters=iters, **{n + '_ms': v for n, v in ms.items()},
                eager_over_topk_lists=round(min(ms['eager']) / best, 2), users_per_s=round(U / best * 1e3),
                gather_GBps=round(U * C * E * 4 / best / 1e6, 1), topk_items_whole_table_ms=round(t_table, 4), id_agreement_with_eager=round(agree, 6))


def eager_mmr(emb, pool_ids, pool_scores, lam, k, chunk):
    """what a caller without the kernel writes: gather the pool's rows of a chunk of users, normalise them, one bmm for the [chunk, P, P] cosine
    matrix, then k rounds of masked argmax and a running maximum over the picked column, driven from the host"""
    ids, scores = [], []
    P = pool_ids.shape[1]
    for a in range(0, pool_ids.shape[0], chunk):
        pid, ps = pool_ids[a:a + chunk].long(), pool_scores[a:a + chunk]
        free = (pid > 0) & torch.isfinite(ps)
        rows = emb[pid]
        rows = rows / rows.norm(dim=2, keepdim=True).clamp_min(1e-30)
        G = torch.bmm(rows, rows.transpose(1, 2))
        lo = torch.where(free, ps, ps.new_full((), float('inf'))).amin(1, keepdim=True)
        hi = torch.where(free, ps, ps.new_full((), -float('inf'))).amax(1, keepdim=True)
        r = torch.where(hi > lo, (ps - lo) / (hi - lo), torch.ones_like(ps))
        m = torch.zeros_like(ps)
        oi = torch.zeros(pid.shape[0], k, dtype=torch.long, device=pid.device)
        os_ = torch.full((pid.shape[0], k), -float('inf'), device=pid.device)
        for t in range(k):
            v = (lam * r - (1.0 - lam) * m).masked_fill(~free, -float('inf'))
            j = v.argmax(1, keepdim=True)
            ok = free.gather(1, j)
            oi[:, t:t + 1] = torch.where(ok, pid.gather(1, j), 0)
            os_[:, t:t + 1] = torch.where(ok, ps.gather(1, j), -float('inf'))
            free.scatter_(1, j, False)
            c = G.gather(1, j[:, :, None].expand(-1, 1, P)).squeeze(1)
            m = c if t == 0 else torch.maximum(m, c)
        ids.append(oi)
        scores.append(os_)
    return torch.cat(ids), torch.cat(scores)


def mmr_cfg(name, U, N1, E, k, P, lam, iters, rounds=2, H=20):
    """--mmr: the pools are a4r_topk_items' P best items of every user; a4r_mmr_rerank and the eager composition on the same pools, interleaved
    `rounds` times, every round's mean reported, the ratio from the minima; a4r_topk_items at K = P, which fills the pool, once for scale."""
    from adapter4rec_amd import _lib as L
    emb, prec, hist, ptr, tgt = data(U, N1, E, H)
    flat = hist.reshape(-1).contiguous()
    pool_i = torch.empty(U, P, dtype=torch.int32, device=DEV)
    pool_s = torch.empty(U, P, dtype=torch.float32, device=DEV)
    t_pool = timed(lambda: L.topk_items(prec, emb, ptr, flat, P, pool_i, pool_s), max(1, iters // 4))
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    ild = torch.empty(U, dtype=torch.float32, device=DEV)
    chunk = max(1, (1 << 28) // (P * max(P, E)))                    # 1 GiB of gathered rows or of cosine matrix per chunk
    legs = dict(mmr_rerank=lambda: L.mmr_rerank(emb, pool_i, pool_s, lam, k, ids, sc, ild), eager=lambda: eager_mmr(emb, pool_i, pool_s, lam, k, chunk))
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters if n == 'mmr_rerank' else max(1, iters // 4)), 4))
    ei, _ = eager_mmr(emb, pool_i, pool_s, lam, k, chunk)
    legs['mmr_rerank']()
    agree = float((ei.int() == ids).all(1).float().mean())          # random fp32 data: the lists agree up to near-ties
    changed = float((ids != pool_i[:, :k]).any(1).float().mean())
    best = min(ms['mmr_rerank'])
    return dict(name=name, users=U, items=N1, E=E, k=k, pool=P, lam=lam, rounds=rounds, iters=iters, **{n + '_ms': v for n, v in ms.items()},
                eager_over_mmr_rerank=round(min(ms['eager']) / best, 2), users_per_s=round(U / best * 1e3),
                row_read_GBps=round(U * k * P * E * 4 / best / 1e6, 1), topk_items_pool_ms=round(t_pool, 4), mean_ild=round(float(ild.mean()), 5),
                lists_equal_to_eager=round(agree, 6), lists_changed_by_mmr=round(changed, 4))


def eager_similar(emb, query, k, chunk=2048):
    """what a caller without the kernel writes: a normalised copy, [chunk, N1] cosines, the pad row and the query itself masked, torch.topk"""
    n = emb / emb.norm(dim=1, keepdim=True).clamp_min(1e-30)
    ids, scores = [], []
    for a in range(0, query.numel(), chunk):
        q = query[a:a + chunk].long()
        s = n[q] @ n.t()
        s[:, 0] = -float('inf')
        s.scatter_(1, q[:, None], -float('inf'))
        v, i = torch.topk(s, k, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def similar_cfg(name, Q, N1, E, k, iters, rounds=3):
    """--similar: the fused entry (inverse norms + a4r_topk_similar), its top-K launch alone, the composition (normalised copy, gather of the query
    rows, a4r_topk_items with one-id exclusion lists; its a4r_topk_items launch alone as well) and eager torch, interleaved `rounds` times after a
    warm-up; every round's mean is reported, the ratios from the minima, and the spread of each leg over its rounds."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(3)
    emb = torch.randn(N1, E, device=DEV, generator=g)
    query = (torch.randperm(N1 - 1, device=DEV, generator=g)[:Q] + 1).to(torch.int32).contiguous()
    ids = torch.empty(Q, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(Q, k, dtype=torch.float32, device=DEV)
    ids_c, sc_c = torch.empty_like(ids), torch.empty_like(sc)
    ptr = torch.arange(Q + 1, device=DEV, dtype=torch.int32)
    inv = L.row_inv_norms(emb)
    normed = (emb * inv[:, None]).contiguous()
    prec = normed[query.long()].contiguous()

    def fused():
        L.topk_similar(emb, L.row_inv_norms(emb), query, None, None, k, ids, sc)

    def composition():
        n = (emb / emb.norm(dim=1, keepdim=True).clamp_min(1e-30)).contiguous()
        L.topk_items(n[query.long()].contiguous(), n, ptr, query, k, ids_c, sc_c)
    legs = dict(similar=fused, similar_topk_only=lambda: L.topk_similar(emb, inv, query, None, None, k, ids, sc), composition=composition,
                composition_topk_only=lambda: L.topk_items(prec, normed, ptr, query, k, ids_c, sc_c), eager=lambda: eager_similar(emb, query, k))
    for fn in legs.values():                                        # warm-up: every leg once before any is timed
        fn()
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters if n != 'eager' else max(1, iters // 4)), 4))
    fused()
    composition()
    ei, _ = eager_similar(emb, query, k)
    spread = {n: round((max(v) - min(v)) / min(v), 4) for n, v in ms.items()}
    best = min(ms['similar'])
    return dict(name=name, queries=Q, items=N1, E=E, k=k, rounds=rounds, iters=iters, **{n + '_ms': v for n, v in ms.items()}, spread=spread,
                similar_over_composition=round(best / min(ms['composition']), 3),
                similar_topk_over_composition_topk=round(min(ms['similar_topk_only']) / min(ms['composition_topk_only']), 3),
                eager_over_similar=round(min(ms['eager']) / best, 2), queries_per_s=round(Q / best * 1e3),
                extra_table_bytes_of_the_composition=N1 * E * 4, id_agreement_with_composition=round(float((ids == ids_c).float().mean()), 6),
                id_agreement_with_eager=round(float((ei.int() == ids).float().mean()), 6))


def bf16_row_sets(E, k):
    """csrc/a4r_topk.hip: topk_bf16_rs -- the 16-user row sets a workgroup of a4r_topk_items_bf16 holds"""
    return 2 if k <= 64 and E in (128, 256) else 1


def bf16_cfg(name, U, N1, E, k, fraction, iters, rounds=3, H=20):
    """--bf16: a4r_topk_items_bf16 beside a4r_topk_items / a4r_topk_items_cand of the same build on the same random data.  Legs, interleaved
    `rounds` times after a warm-up of each: fp32; bf16 (operands cast beforehand); bf16_cast (the table's and the users' casts inside the timed
    region).  Per leg every round's mean, the minimum's ratio and the spread (max - min) / min; the table bytes per second (table bytes x passes:
    one pass per 16 users in fp32, per 16 x row sets in bf16; at K >= 100 the time goes to sort-and-cut rounds as well) and the bf16 leg's share
    of the 2.5 PF bf16 MFMA peak; and how the two lists differ on this data (logged, not asserted): the share of users whose lists are identical,
    and the share of list positions holding the same id."""
    from adapter4rec_amd import _lib as L
    emb, prec, hist, ptr, tgt = data(U, N1, E, H)
    flat = hist.reshape(-1).contiguous()
    cand = None
    if fraction is not None:
        g = torch.Generator(device=DEV).manual_seed(1)
        cand = (torch.rand(N1, device=DEV, generator=g) < fraction).to(torch.uint8).contiguous()
    emb_b = torch.empty(N1, E, dtype=torch.bfloat16, device=DEV)
    prec_b = torch.empty(U, E, dtype=torch.bfloat16, device=DEV)
    L.cast_bf16(emb, emb_b)
    L.cast_bf16(prec, prec_b)
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    ids_b, sc_b = torch.empty_like(ids), torch.empty_like(sc)

    def fp32():
        L.topk_items(prec, emb, ptr, flat, k, ids, sc) if cand is None else L.topk_items_cand(prec, emb, ptr, flat, cand, k, ids, sc)

    def bf16():
        L.topk_items_bf16(prec_b, emb_b, ptr, flat, k, ids_b, sc_b, cand)

    def bf16_cast():
        L.cast_bf16(emb, emb_b)
        L.cast_bf16(prec, prec_b)
        L.topk_items_bf16(prec_b, emb_b, ptr, flat, k, ids_b, sc_b, cand)
    legs = dict(fp32=fp32, bf16=bf16, bf16_cast=bf16_cast)
    for fn in legs.values():                                        # warm-up: every leg once before any is timed
        fn()
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters), 4))
    best = {n: min(v) for n, v in ms.items()}
    spread = {n: round((max(v) - min(v)) / min(v), 4) for n, v in ms.items()}
    rs = bf16_row_sets(E, k)
    return dict(bench='topk', name=name, box=torch.cuda.get_device_name(0), users=U, items=N1, E=E, k=k, fraction=fraction, rounds=rounds, iters=iters,
                row_sets=rs, **{n + '_ms': v for n, v in ms.items()}, spread=spread, fp32_over_bf16=round(best['fp32'] / best['bf16'], 2),
                fp32_over_bf16_cast=round(best['fp32'] / best['bf16_cast'], 2),
                fp32_table_TB_per_s=round(N1 * E * 4 * ((U + 15) // 16) / best['fp32'] / 1e9, 2),
                bf16_table_TB_per_s=round(N1 * E * 2 * ((U + 16 * rs - 1) // (16 * rs)) / best['bf16'] / 1e9, 2),
                bf16_share_of_mfma_peak=round(2.0 * U * N1 * E / best['bf16'] / 1e9 / 2500.0, 4),
                identical_lists=round(float((ids == ids_b).all(1).float().mean()), 4), same_id_positions=round(float((ids == ids_b).float().mean()), 4))


def eager_audience(item, query, users, seen, k, chunk=512):
    """what a caller without the kernel writes: the (query, user row) pairs of the seen lists through a lookup of the query items, [chunk, U1]
    scores, the pad row and the seen pairs set to -inf, torch.topk"""
    pos = torch.full((item.shape[0],), -1, dtype=torch.long, device=item.device)
    pos[query.long()] = torch.arange(query.numel(), device=item.device)
    qp = pos[seen.long().reshape(-1)]
    row = torch.arange(1, users.shape[0], device=item.device).repeat_interleave(seen.shape[1])
    qp, row = qp[qp >= 0], row[qp >= 0]
    rows, scores = [], []
    for a in range(0, query.numel(), chunk):
        s = item[query[a:a + chunk].long()] @ users.t()
        s[:, 0] = -float('inf')
        m = (qp >= a) & (qp < a + chunk)
        s[qp[m] - a, row[m]] = -float('inf')
        v, i = torch.topk(s, k, dim=1)
        rows.append(i)
        scores.append(v)
    return torch.cat(rows), torch.cat(scores)


def audience_cfg(name, Q, N1, U1, E, k, iters, rounds=3, H=20):
    """--audience: a4r_topk_users, the same launch with every seen list empty (what the launch costs without the probes of the lists), the
    role-swapped a4r_topk_items with empty exclusion lists (the nearest existing launch) and eager torch, interleaved `rounds` times after a warm-up; every round's mean is reported, the ratios from the minima, and the spread of each leg over its
    rounds."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(5)
    item = torch.randn(N1, E, device=DEV, generator=g)
    users = torch.randn(U1, E, device=DEV, generator=g)
    users[0] = 0
    query = (torch.randperm(N1 - 1, device=DEV, generator=g)[:Q] + 1).to(torch.int32).contiguous()
    seen = torch.randint(1, N1, (U1 - 1, H), device=DEV, generator=g, dtype=torch.int32).sort(dim=1).values.contiguous()      # ascending within a row
    sptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.arange(U1, device=DEV, dtype=torch.int64) * H]).contiguous()      # row 0 empty
    flat = seen.reshape(-1)
    rows = torch.empty(Q, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(Q, k, dtype=torch.float32, device=DEV)
    rows_s, sc_s = torch.empty_like(rows), torch.empty_like(sc)
    prec = item[query.long()].contiguous()
    ptr0 = torch.zeros(Q + 1, dtype=torch.int32, device=DEV)
    none = torch.zeros(1, dtype=torch.int32, device=DEV)
    sptr0 = torch.zeros(U1 + 1, dtype=torch.int64, device=DEV)
    rows_n, sc_n = torch.empty_like(rows), torch.empty_like(sc)
    legs = dict(users=lambda: L.topk_users(item, query, users, sptr, flat, None, k, rows, sc),
                users_empty_lists=lambda: L.topk_users(item, query, users, sptr0, flat, None, k, rows_n, sc_n),      # the two offsets are loaded, no list is probed
                swapped=lambda: L.topk_items(prec, users, ptr0, none, k, rows_s, sc_s), eager=lambda: eager_audience(item, query, users, seen, k))
    for fn in legs.values():                                        # warm-up: every leg once before any is timed
        fn()
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, iters if n != 'eager' else max(1, iters // 4)), 4))
    legs['users']()
    legs['swapped']()
    ei, _ = eager_audience(item, query, users, seen, k)
    torch.cuda.synchronize()
    spread = {n: round((max(v) - min(v)) / min(v), 4) for n, v in ms.items()}
    best = min(ms['users'])
    return dict(name=name, queries=Q, items=N1, user_rows=U1, seen_per_user=H, E=E, k=k, rounds=rounds, iters=iters, **{n + '_ms': v for n, v in ms.items()},
                spread=spread, users_over_swapped=round(best / min(ms['swapped']), 3),
                users_empty_lists_over_swapped=round(min(ms['users_empty_lists']) / min(ms['swapped']), 3), eager_over_users=round(min(ms['eager']) / best, 2),
                queries_per_s=round(Q / best * 1e3), lists_differing_from_swapped=int((rows != rows_s).any(1).sum()),
                row_agreement_with_eager=round(float((ei.int() == rows).float().mean()), 6))


def eager_exclude(prec, emb, lists, k, chunk=2048):
    """what a caller without the kernel writes for lists of any length: [chunk, N1] scores, the pad row and the listed pairs set to -inf, topk"""
    ids, scores = [], []
    for a in range(0, prec.shape[0], chunk):
        s = prec[a:a + chunk] @ emb.t()
        s[:, 0] = -float('inf')
        s.scatter_(1, lists[a:a + chunk].long(), -float('inf'))
        v, i = torch.topk(s, k, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids), torch.cat(scores)


def own_best(prec, emb, n, chunk=2048):
    """every user's n highest-scoring items, ascending by id: the hard case of an exclusion list -- exactly the keys that beat the threshold"""
    out = []
    for a in range(0, prec.shape[0], chunk):
        s = prec[a:a + chunk] @ emb.t()
        s[:, 0] = -float('inf')
        out.append(torch.topk(s, n, dim=1).indices.to(torch.int32).sort(dim=1).values)
    return torch.cat(out).contiguous()


def exclude_cfg(name, U, N1, E, k, iters, rounds=3):
    """--exclude: (a) a4r_topk_items_excl beside a4r_topk_items of the same build on identical lists of 20 and of 264 ids (both entries serve
    them); (b) a4r_topk_items_excl at 1 000 and 5 000 ids per user beside eager torch, the lists drawn uniformly and as the user's own best items.
    All legs interleaved `rounds` times after a warm-up of each; every round's mean is reported, the ratios from the minima, and the spread of each
    leg over its rounds."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator(device=DEV).manual_seed(7)
    emb = torch.randn(N1, E, device=DEV, generator=g)
    prec = torch.randn(U, E, device=DEV, generator=g)
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    ids_x, sc_x = torch.empty_like(ids), torch.empty_like(sc)
    legs, eager, checks = {}, set(), {}
    for H in (20, 264):
        lists = torch.randint(1, N1, (U, H), device=DEV, generator=g, dtype=torch.int32).sort(dim=1).values.contiguous()      # ascending within a user
        p32 = (torch.arange(U + 1, device=DEV, dtype=torch.int32) * H).contiguous()
        p64 = p32.long().contiguous()
        flat = lists.reshape(-1)
        legs[f'items_h{H}'] = (lambda p=p32, f=flat: L.topk_items(prec, emb, p, f, k, ids, sc))
        legs[f'excl_h{H}'] = (lambda p=p64, f=flat: L.topk_items_excl(prec, emb, p, f, None, k, ids_x, sc_x))
        checks[f'h{H}'] = (f'items_h{H}', f'excl_h{H}')
    for H in (1000, 5000):
        for draw in ('uniform', 'top'):
            lists = (torch.randint(1, N1, (U, H), device=DEV, generator=g, dtype=torch.int32).sort(dim=1).values.contiguous() if draw == 'uniform'
                     else own_best(prec, emb, H))
            p64 = (torch.arange(U + 1, device=DEV, dtype=torch.int64) * H).contiguous()
            legs[f'excl_{draw}{H}'] = (lambda p=p64, f=lists.reshape(-1): L.topk_items_excl(prec, emb, p, f, None, k, ids_x, sc_x))
            legs[f'eager_{draw}{H}'] = (lambda l=lists: eager_exclude(prec, emb, l, k))
            eager.add(f'eager_{draw}{H}')
            checks[f'{draw}{H}'] = (f'eager_{draw}{H}', f'excl_{draw}{H}')
    for fn in legs.values():                                        # warm-up: every leg once before any is timed
        fn()
    ms = {n: [] for n in legs}
    for _ in range(rounds):
        for n, fn in legs.items():
            ms[n].append(round(timed(fn, max(1, iters // 4) if n in eager else iters), 4))
    agree = {}
    for what, (ref, new) in checks.items():                         # equal lists on the lists both entries serve; up to near-ties against eager
        r = legs[ref]()
        legs[new]()
        torch.cuda.synchronize()
        agree[what] = round(float((r[0].int() == ids_x).float().mean()), 6)
    best = {n: min(v) for n, v in ms.items()}
    spread = {n: round((max(v) - min(v)) / min(v), 4) for n, v in ms.items()}
    ratios = {f'excl_over_items_h{H}': round(best[f'excl_h{H}'] / best[f'items_h{H}'], 3) for H in (20, 264)}
    ratios.update({f'eager_over_excl_{d}{H}': round(best[f'eager_{d}{H}'] / best[f'excl_{d}{H}'], 2) for H in (1000, 5000) for d in ('uniform', 'top')})
    ratios.update({f'excl_{d}{H}_over_excl_h20': round(best[f'excl_{d}{H}'] / best['excl_h20'], 3) for H in (1000, 5000) for d in ('uniform', 'top')})
    return dict(bench='topk', name=name, box=torch.cuda.get_device_name(0), users=U, items=N1, E=E, k=k, rounds=rounds, iters=iters,
                **{n + '_ms': v for n, v in ms.items()}, spread=spread, **ratios, id_agreement=agree)


def recommend_cfg(name, U, item_num, k, iters, T=20):
    from adapter4rec_amd.cv import Model
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import recommend
    args = argparse.Namespace(max_seq_len=T, l2_weight=0, embedding_dim=64, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                              CV_model_load='vit-base-patch16-224', compute_dtype='bf16', arch='sasrec', adapter_type='None')
    model = Model(args, item_num, False, None).to(DEV)
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    rng = np.random.default_rng(0)
    seqs = {u: list(rng.integers(1, item_num + 1, size=T + 3)) for u in range(U)}
    recommend(model, seqs, emb, k, args)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ids, _ = recommend(model, seqs, emb, k, args)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return dict(name=name, users=U, items=item_num + 1, E=64, k=k, recommend_ms=round(dt * 1e3, 2), users_per_s=round(U / dt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--only', default=None)
    ap.add_argument('--candidates', type=float, default=None, metavar='FRACTION',
                    help='run the candidate-set leg instead: the masked entries beside the unmasked ones under a random mask of this fraction')
    ap.add_argument('--lists', type=int, default=None, metavar='C', choices=(0, 100, 1000, 4096),
                    help="run the per-user-list leg instead: a4r_topk_lists over C listed items per user beside the eager gather path (0: every C)")
    ap.add_argument('--mmr', action='store_true',
                    help='run the re-ranking leg instead: a4r_mmr_rerank beside the eager gather + bmm + K-round loop, pools of 100 and 256, E = 64 and 128')
    ap.add_argument('--similar', action='store_true',
                    help='run the similar-items leg instead: a4r_topk_similar beside the composition of existing entries and eager torch, K = 10 and 100, E = 64 and 128')
    ap.add_argument('--bf16', action='store_true',
                    help='run the bf16-score leg instead: a4r_topk_items_bf16 beside the fp32 entries, K = 10 / 100 / 256, E = 64 .. 512, candidates off and at 0.1')
    ap.add_argument('--audience', action='store_true',
                    help='run the audience leg instead: a4r_topk_users beside the role-swapped a4r_topk_items and eager torch, K = 10 and 100, E = 64 and 128')
    ap.add_argument('--exclude', action='store_true',
                    help='run the exclusion-list leg instead: a4r_topk_items_excl beside a4r_topk_items (20 / 264 ids) and eager torch (1 000 / 5 000 ids), K = 10 and 100, E = 64 and 128')
    a = ap.parse_args()
    if a.exclude:
        for k in (10, 100):
            for E in (64, 128):
                name = f'exclude_k{k}_e{E}'
                if not a.only or a.only == name:
                    print(json.dumps(exclude_cfg(name, 32768, 65537, E, k, a.iters)), flush=True)
        return
    if a.audience:
        for k in (10, 100):
            for E in (64, 128):
                name = f'audience_k{k}_e{E}'
                if not a.only or a.only == name:
                    print(json.dumps(audience_cfg(name, 4096, 65537, 262145, E, k, a.iters)), flush=True)
        return
    if a.bf16:
        for N1, widths, it in ((65537, (64, 128, 256, 512), a.iters), (500001, (64, 128), max(1, a.iters // 4))):
            for E in widths:
                for k in (10, 100, 256):
                    for fraction in (None, 0.1):
                        name = f'bf16_k{k}_e{E}_{N1}' + ('' if fraction is None else '_cand')
                        if not a.only or a.only == name:
                            print(json.dumps(bf16_cfg(name, 32768, N1, E, k, fraction, it)), flush=True)
        return
    if a.similar:
        for k in (10, 100):
            for E in (64, 128):
                name = f'similar_k{k}_e{E}'
                if not a.only or a.only == name:
                    print(json.dumps(similar_cfg(name, 32768, 65537, E, k, a.iters)), flush=True)
        return
    if a.mmr:
        for P in (100, 256):
            for E in (64, 128):
                name = f'mmr_p{P}_e{E}'
                if not a.only or a.only == name:
                    print(json.dumps(mmr_cfg(name, 32768, 65537, E, 10, P, 0.7, a.iters)), flush=True)
        return
    if a.lists is not None:
        for C in ((100, 1000, 4096) if a.lists == 0 else (a.lists,)):
            for E in (64, 128):
                name = f'lists_c{C}_e{E}'
                if not a.only or a.only == name:
                    print(json.dumps(lists_cfg(name, 32768, 65537, E, 10, C, a.iters if C < 4096 else max(2, a.iters // 4))), flush=True)
        return
    if a.candidates is not None:
        for name, N1, it in (('cand_k10_65537', 65537, a.iters), ('cand_k10_500000', 500000, max(1, a.iters // 4))):
            if not a.only or a.only == name:
                print(json.dumps(cand_cfg(name, 32768, N1, 64, 10, a.candidates, it)), flush=True)
        return
    cfgs = [
        ('k10_65537', lambda: kernel_cfg('k10_65537', 32768, 65537, 64, 10, a.iters)),
        ('k100_65537', lambda: kernel_cfg('k100_65537', 32768, 65537, 64, 100, a.iters)),
        ('k10_500001', lambda: kernel_cfg('k10_500001', 32768, 500001, 64, 10, max(1, a.iters // 4))),
        ('k100_500001', lambda: kernel_cfg('k100_500001', 32768, 500001, 64, 100, max(1, a.iters // 4))),
        ('recommend_k10_65537', lambda: recommend_cfg('recommend_k10_65537', 32768, 65536, 10, 3)),
    ]
    for name, fn in cfgs:
        if a.only and a.only != name:
            continue
        print(json.dumps(fn()), flush=True)


if __name__ == '__main__':
    main()
