#!/usr/bin/env python
"""Throughput of the native evaluation (reference: Downstream/Text/data_utils/metrics.py:62-116).

  python tools/eval_bench.py [--items 65536] [--users 32768] [--json out.json] [--candidates FRACTION] [--sampled N [N ...]] [--bf16]

--candidates FRACTION runs the candidate-set leg instead (candidates_leg): a4r_eval_rank_cand beside a4r_eval_rank, kernels only.
--sampled N [N ...] runs the sampled-evaluation leg instead (sampled_leg): a4r_eval_rank_sampled beside the two-launch composition
(a4r_eval_draw_negatives + a4r_eval_rank_lists), the full sweep a4r_eval_rank and an eager torch path, kernels only; one JSON line per
configuration, appended to --json (the numbers land in profiles/eval_negatives_bench.jsonl).
--bf16 runs the bf16-score leg instead (bf16_leg): a4r_eval_rank_bf16 beside the fp32 entries of the same build, kernels only, the casts in one
leg and outside another; one JSON line per configuration, appended to --json (the numbers land in profiles/score_bf16_bench.jsonl).

Times, on one MI355X, with BERT-base + Houlsby weights (random init, as bench.py):
  * the item sweep `get_item_embeddings` (all N + 1 titles through the item encoder, forward only) in the eval dtypes
    (--eval_compute_dtype fp32 = the default: exact-fp32 MFMA; bf16), at run.py's batch of 512 titles and at 4 096;
  * `eval_model`: user encoder + a4r_eval_rank over `users` users at run.py's batch of 512 users, and the rank kernel alone
    (HIP events) against its HBM/L2 roofline: the kernel streams the N x E fp32 item table once per 16 users.
Prints one JSON object; the numbers land in profiles/r03_*_eval_bench.json."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def candidates_leg(a, dev):
    """--candidates FRACTION: the rank kernel alone on a random [items + 1, 64] table -- a4r_eval_rank_cand under a random candidate set of that
    fraction of the items beside a4r_eval_rank on the same data, interleaved over two rounds (no encoder: the set concerns the rank kernel only)."""
    from adapter4rec_amd import _lib as L
    E, N1 = 64, a.items + 1
    g = torch.Generator(device=dev).manual_seed(B.SEED)
    emb = torch.randn(N1, E, device=dev, generator=g)
    cand = (torch.rand(N1, device=dev, generator=g) < a.candidates).to(torch.uint8).contiguous()
    res = dict(items=N1, E=E, fraction=a.candidates, candidates=int(cand[1:].ne(0).sum()))
    for U in (512, 4096, 32768):
        prec = torch.randn(U, E, device=dev, generator=g)
        target = torch.randint(1, N1, (U,), device=dev, dtype=torch.int32, generator=g)
        ptr = torch.arange(0, U + 1, device=dev, dtype=torch.int32) * 20
        hidx = torch.randint(1, N1, (U * 20 + 1,), device=dev, dtype=torch.int32, generator=g)
        rank = torch.zeros(U, dtype=torch.int32, device=dev)
        legs = dict(eval_rank=lambda: L.eval_rank(prec, emb, target, ptr, hidx, rank),
                    eval_rank_cand=lambda: L.eval_rank_cand(prec, emb, target, ptr, hidx, cand, rank))
        us = {n: [] for n in legs}
        for _ in range(2):
            for n, fn in legs.items():
                for _ in range(2):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[n].append(round(e0.elapsed_time(e1) / 10 * 1e3, 1))
        res[f'U{U}'] = dict(eval_rank_us=us['eval_rank'], eval_rank_cand_us=us['eval_rank_cand'],
                            cand_over_plain=round(min(us['eval_rank_cand']) / min(us['eval_rank']), 3))
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)


def sampled_leg(a, dev):
    """--sampled N [N ...]: ranking every user's target among N negatives drawn on the device, E = 64 and 128, uniform and popularity sampling, on
    random tables of items + 1 rows and histories of 20 ids.  Four ways, interleaved over ``rounds`` rounds after a warm-up of each, the minimum
    of the rounds reported (device events around ``reps`` calls):
      fused     a4r_eval_rank_sampled: one launch, nothing of size U x N in memory
      two       a4r_eval_draw_negatives + a4r_eval_rank_lists: the draws materialised [U, N] and read back as a CSR -- the figure to beat
      sweep     a4r_eval_rank: the rank among ALL items (another protocol: what the sampling saves or costs)
      eager     torch: randint negatives (no exclusion, another stream of draws) + gather + einsum + compare
    fused and two must give the same ranks: checked on every configuration before anything is timed."""
    from adapter4rec_amd import _lib as L
    N1, U, rounds, reps = a.items + 1, a.users, 5, 5
    g = torch.Generator(device=dev).manual_seed(B.SEED)
    box = torch.cuda.get_device_name(0)
    out = open(a.json, 'a') if a.json else None
    for E in (64, 128):
        emb = torch.randn(N1, E, device=dev, generator=g)
        prec = torch.randn(U, E, device=dev, generator=g)
        target = torch.randint(1, N1, (U,), device=dev, dtype=torch.int32, generator=g)
        ptr = torch.arange(0, U + 1, device=dev, dtype=torch.int32) * 20
        hidx = torch.randint(1, N1, (U * 20 + 1,), device=dev, dtype=torch.int32, generator=g)
        keys = torch.arange(U, device=dev, dtype=torch.int32)
        cnt = torch.randint(0, 1000, (N1,), device=dev, generator=g) ** 2 // 1000          # a skewed popularity, a tenth of the items near 0
        cnt[0] = 0
        pop_cdf = torch.cumsum(cnt, 0).to(torch.int64).contiguous()
        rank = torch.zeros(U, dtype=torch.int32, device=dev)
        rank2 = torch.zeros(U, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        for n in a.sampled:
            ids = torch.zeros(U, n, dtype=torch.int32, device=dev)
            lptr = torch.arange(0, U + 1, device=dev, dtype=torch.int32) * n
            for sampling, cdf in (('uniform', None), ('pop', pop_cdf)):
                def fused():
                    L.eval_rank_sampled(prec, emb, target, ptr, hidx, keys, cdf, B.SEED, n, rank, err)

                def two():
                    L.eval_draw_negatives(ptr, hidx, target, keys, cdf, B.SEED, N1, ids, err)
                    L.eval_rank_lists(prec, emb, target, lptr, ids.view(-1), n, ptr, hidx, rank2)

                def sweep():
                    L.eval_rank(prec, emb, target, ptr, hidx, rank2)

                def eager():
                    neg = torch.randint(1, N1, (U, n), device=dev)
                    s = torch.einsum('ue,une->un', prec, emb[neg])
                    t = (prec * emb[target.long()]).sum(1, keepdim=True)
                    return 1 + (s > t).sum(1)
                fused()
                two()
                torch.cuda.synchronize()
                assert torch.equal(rank, rank2) and int(err.item()) == 0, 'the fused entry and the two-launch composition disagree'
                legs = dict(fused=fused, two=two, sweep=sweep, eager=eager)
                us = {k: [] for k in legs}
                for fn in legs.values():
                    fn()
                    fn()
                for _ in range(rounds):
                    for k, fn in legs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            fn()
                        e1.record()
                        torch.cuda.synchronize()
                        us[k].append(round(e0.elapsed_time(e1) / reps * 1e3, 1))
                best = {k: min(v) for k, v in us.items()}
                line = dict(box=box, items=N1, users=U, E=E, N=n, sampling=sampling, rounds=rounds, reps=reps,
                            fused_us=best['fused'], two_launch_us=best['two'], sweep_us=best['sweep'], eager_us=best['eager'], all_us=us,
                            fused_over_two_launch=round(best['fused'] / best['two'], 3), fused_users_per_s=round(U / best['fused'] * 1e6, 1),
                            gathered_GB_per_s=round(U * (n + 1) * E * 4 / best['fused'] / 1e3, 1), mean_rank=round(float(rank.float().mean()), 2))
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + '\n')
                    out.flush()


BF16_RANK_ROW_SETS = {64: 8, 128: 8, 256: 4, 512: 2}      # csrc/a4r_eval.hip: RankBf16Shape -- 16-user row sets a workgroup of a4r_eval_rank_bf16 holds
BF16_PEAK_TF = 2500.0


def bf16_leg(a, dev):
    """--bf16: a4r_eval_rank_bf16 beside a4r_eval_rank / a4r_eval_rank_cand of the same build on the same random tables, kernels only: 32 768 users
    (--users), 65 537 items at E = 64 .. 512 and 500 001 items at E = 64 / 128, the candidate set off and at 0.1.  Legs, interleaved over three
    rounds after a warm-up of each, device events around ``reps`` calls: fp32; bf16 (operands cast beforehand); bf16_cast (the table's and the
    users' casts inside the timed region: what one evaluation batch pays).  Per leg the minimum and the spread (max - min) / min of the rounds,
    the table bytes per second (table bytes x passes: one pass per 16 users in fp32, per 16 x row sets in bf16) and, for bf16, the share of the
    2.5 PF bf16 MFMA peak.  Also the agreement of the two on the same data: largest |rank change|, HR@10 / nDCG@10 of both (logged, not asserted).
    One JSON line per configuration, appended to --json."""
    from adapter4rec_amd import _lib as L
    U, rounds = a.users, 3
    g = torch.Generator(device=dev).manual_seed(B.SEED)
    box = torch.cuda.get_device_name(0)
    out = open(a.json, 'a') if a.json else None
    for N1, E in ((65537, 64), (65537, 128), (65537, 256), (65537, 512), (500001, 64), (500001, 128)):
        reps = 5 if N1 < 100000 else 2
        emb = torch.randn(N1, E, device=dev, generator=g)
        prec = torch.randn(U, E, device=dev, generator=g)
        target = torch.randint(1, N1, (U,), device=dev, dtype=torch.int32, generator=g)
        ptr = torch.arange(0, U + 1, device=dev, dtype=torch.int32) * 20
        hidx = torch.randint(1, N1, (U * 20 + 1,), device=dev, dtype=torch.int32, generator=g)
        emb_b = torch.empty(N1, E, dtype=torch.bfloat16, device=dev)
        prec_b = torch.empty(U, E, dtype=torch.bfloat16, device=dev)
        L.cast_bf16(emb, emb_b)
        L.cast_bf16(prec, prec_b)
        r32 = torch.zeros(U, dtype=torch.int32, device=dev)
        rb = torch.zeros(U, dtype=torch.int32, device=dev)
        for fraction in (None, 0.1):
            cand = None if fraction is None else (torch.rand(N1, device=dev, generator=g) < fraction).to(torch.uint8).contiguous()

            def fp32():
                L.eval_rank(prec, emb, target, ptr, hidx, r32) if cand is None else L.eval_rank_cand(prec, emb, target, ptr, hidx, cand, r32)

            def bf16():
                L.eval_rank_bf16(prec_b, emb_b, target, ptr, hidx, rb, cand)

            def bf16_cast():
                L.cast_bf16(emb, emb_b)
                L.cast_bf16(prec, prec_b)
                L.eval_rank_bf16(prec_b, emb_b, target, ptr, hidx, rb, cand)
            legs = dict(fp32=fp32, bf16=bf16, bf16_cast=bf16_cast)
            for fn in legs.values():
                fn()
                fn()
            us = {k: [] for k in legs}
            for _ in range(rounds):
                for k, fn in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[k].append(round(e0.elapsed_time(e1) / reps * 1e3, 1))
            best = {k: min(v) for k, v in us.items()}
            spread = {k: round((max(v) - min(v)) / min(v), 4) for k, v in us.items()}
            a32, ab = r32.float(), rb.float()
            metrics = lambda r: [round(float((r <= 10).float().mean()), 6), round(float(torch.where(r <= 10, 1 / torch.log2(r + 1), torch.zeros_like(r)).mean()), 6)]
            passes32, passes_b = (U + 15) // 16, (U + 16 * BF16_RANK_ROW_SETS[E] - 1) // (16 * BF16_RANK_ROW_SETS[E])
            line = dict(bench='eval_rank', box=box, users=U, items=N1, E=E, fraction=fraction, rounds=rounds, reps=reps, row_sets=BF16_RANK_ROW_SETS[E],
                        fp32_us=best['fp32'], bf16_us=best['bf16'], bf16_cast_us=best['bf16_cast'], all_us=us, spread=spread,
                        fp32_over_bf16=round(best['fp32'] / best['bf16'], 2), fp32_over_bf16_cast=round(best['fp32'] / best['bf16_cast'], 2),
                        fp32_table_TB_per_s=round(N1 * E * 4 * passes32 / best['fp32'] / 1e6, 2),
                        bf16_table_TB_per_s=round(N1 * E * 2 * passes_b / best['bf16'] / 1e6, 2),
                        bf16_share_of_mfma_peak=round(2.0 * U * N1 * E / best['bf16'] / 1e6 / BF16_PEAK_TF, 4),
                        ranks_equal=round(float((r32 == rb).float().mean()), 4), largest_rank_change=int((r32 - rb).abs().max()),
                        median_rank_change=float((a32 - ab).abs().median()), hr10_ndcg10_fp32=metrics(a32), hr10_ndcg10_bf16=metrics(ab))
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + '\n')
                out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=65536)
    ap.add_argument('--users', type=int, default=32768)
    ap.add_argument('--json', default='')
    ap.add_argument('--candidates', type=float, default=None, metavar='FRACTION',
                    help='run the candidate-set leg instead: a4r_eval_rank_cand beside a4r_eval_rank under a random mask of this fraction')
    ap.add_argument('--sampled', type=int, nargs='+', default=None, metavar='N',
                    help='run the sampled-evaluation leg instead: a4r_eval_rank_sampled beside draw + rank_lists, the full sweep and eager torch, at N negatives')
    ap.add_argument('--bf16', action='store_true',
                    help='run the bf16-score leg instead: a4r_eval_rank_bf16 beside a4r_eval_rank / a4r_eval_rank_cand, with and without the casts')
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    if a.bf16:
        return bf16_leg(a, dev)
    if a.candidates is not None:
        return candidates_leg(a, dev)
    if a.sampled is not None:
        return sampled_leg(a, dev)
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd.data_utils import eval_model, get_item_embeddings
    args = B.make_args(32, 'bf16')
    model, _ = B.build_model(args, dev)
    model.eval()
    g = torch.Generator().manual_seed(B.SEED)
    content = B.synth_content(a.items, g).numpy()
    res = dict(items=a.items + 1, tokens_per_item=30, encoder='BERT-base + Houlsby (random init)', sweep={})
    # forward FLOPs per item: 12 layers x 30 tokens x (2 x 14 155 776 dense + attention 4 S H) + adapters 2 x 2 x 2 x 768 x 64
    flop_item = 12 * 30 * (2 * 7077888 + 4 * 30 * 768 + 2 * 2 * 2 * 768 * 64)
    emb = None
    for dt in ('fp32', 'bf16'):
        for bs in (512, 4096):
            args.eval_compute_dtype = dt
            get_item_embeddings(model, content[:bs * 2], bs, args, True, 0)             # warm-up: snapshot engine build + buffers
            t, e = timed(lambda: get_item_embeddings(model, content, bs, args, True, 0))
            peak = 157.3 if dt == 'fp32' else 2500.0
            res['sweep'][f'{dt}_batch{bs}'] = dict(seconds=round(t, 3), items_per_s=round((a.items + 1) / t, 1),
                                                   tflops=round((a.items + 1) * flop_item / t / 1e12, 1),
                                                   frac_of_mfma_peak=round((a.items + 1) * flop_item / t / 1e12 / peak, 3), peak_tflops=peak)
            if dt == 'fp32' and bs == 512:
                emb = e
    # users: random histories of 5..22 items, the last one held out
    rng = np.random.default_rng(B.SEED)
    eval_seq, hist = {}, {}
    for u in range(a.users):
        n = int(rng.integers(5, 22))                                # <= max_seq_len + 1 = 21 (data_utils/preprocess.py:48-59)
        seq = [int(x) for x in rng.integers(1, a.items + 1, size=n)]
        eval_seq[u], hist[u] = seq, torch.LongTensor(seq[:-1])
    log = logging.getLogger('eval-bench')
    eval_model(model, {u: hist[u] for u in range(1024)}, {u: eval_seq[u] for u in range(1024)}, emb, 512, args, a.items, log, 'valid', 0)
    t, hr = timed(lambda: eval_model(model, hist, eval_seq, emb, 512, args, a.items, log, 'valid', 0))
    res['eval_model'] = dict(users=a.users, batch=512, seconds=round(t, 3), users_per_s=round(a.users / t, 1), hr10=hr,
                             note='first evaluation of these users: includes building the evaluation set (ids, masks, history CSR) from the two dicts')
    t2, hr2 = timed(lambda: eval_model(model, hist, eval_seq, emb, 512, args, a.items, log, 'valid', 0), reps=3)
    res['eval_model_repeat'] = dict(users=a.users, seconds=round(t2, 4), users_per_s=round(a.users / t2, 1), hr10=hr2,
                                    note='every later evaluation of a run (run.py evaluates the same users each epoch: the set is cached on the device)')
    # the rank kernel alone
    E = emb.shape[1]
    for U in (512, 4096, 32768):
        prec = torch.randn(U, E, device=dev)
        target = torch.randint(1, a.items + 1, (U,), device=dev, dtype=torch.int32)
        ptr = torch.arange(0, U + 1, device=dev, dtype=torch.int32) * 20
        hidx = torch.randint(1, a.items + 1, (U * 20 + 1,), device=dev, dtype=torch.int32)
        rank = torch.zeros(U, dtype=torch.int32, device=dev)
        for _ in range(2):
            L.eval_rank(prec, emb, target, ptr, hidx, rank)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            L.eval_rank(prec, emb, target, ptr, hidx, rank)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 10 * 1e3
        table_bytes = (a.items + 1) * E * 4
        streamed = table_bytes * ((U + 15) // 16)                   # algorithmic: the table once per 16 users (from L2 / Infinity Cache / HBM)
        res[f'eval_rank_U{U}'] = dict(us=round(us, 1), users_per_s=round(U / us * 1e6, 1), table_MB=round(table_bytes / 1e6, 1),
                                      streamed_GB_per_s=round(streamed / us / 1e3, 1), flops_TF=round(2.0 * U * (a.items + 1) * E / us / 1e6, 2),
                                      note='table is 16.8 MB: Infinity-Cache resident; bound = L2/MALL bandwidth and the fp32 MFMA rate (157 TF)')
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
