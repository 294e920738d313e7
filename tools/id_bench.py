#!/usr/bin/env python
"""Throughput of the ID item tower (--item_tower id, the IDRec baseline) on its public path: optimizer.zero_grad(), model(ids, log_mask),
loss.backward(), FusedAdam.step() -- one JSON line per configuration (ms/step, user-seq/s, and the inverted index's list lengths of a batch).

    python tools/id_bench.py [--steps K] [--warmup W] [--only NAME] [--loss {bce,ce}] [--ce_dtype {fp32,bf16}] [--skip_eager]

Configurations (the reference's CV defaults: B 64, E 64, 2 blocks x 2 heads, Downstream/CV/parameters.py):
  full_L10 / full_L20     full histories at --max_seq_len 10 / 20, item_num 14 720 (the Amazon 2w catalogue), ids uniform
  real_L20                the 1 024 real user sequences of tests/golden/real_data/amazon_users_head.tsv (real lengths, real repeats), 64 per batch
  full_L20_500k           item_num 500 000: what dense Adam and zero_grad cost over a large table
--loss ce trains with the softmax cross-entropy over the whole table (a4r_score_ce_*) and adds, per configuration, a second JSON line that times
the head alone (forward + both backward launches on the step's own rows and table) beside the same head in eager fp32 torch.matmul +
F.cross_entropy (forward + backward), with torch.cuda.max_memory_allocated of each above what was allocated before it ran.
--ce_dtype bf16 (with --loss ce) trains with the head on the bf16 MFMA (a4r_score_ce_bf16_*); the head-alone line then times those entry points,
the two cast launches (table and rows) counted in fused_ms and reported on their own as cast_ms.  --skip_eager leaves the eager head out.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/id_bench.py`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, E = 64, 64
FP32_MFMA_PEAK = 157.3e12   # flop/s, MI355X fp32 matrix peak: the per-launch fractions of --loss ce are relative to it


def model_args(max_seq_len):
    return argparse.Namespace(max_seq_len=max_seq_len, l2_weight=0, embedding_dim=E, num_attention_heads=2, drop_rate=0.1, transformer_block=2,
                              CV_model_load='vit-base-patch16-224', compute_dtype='bf16', arch='sasrec')


def batch_from_seqs(seqs, L, item_num, rng):
    """BuildTrainDataset(use_modal=False) for a list of user sequences (left padded, one uniform negative per real position outside the
    user's sequence) -> (host int64 ids [B * L * 2], host log_mask [B, L - 1])."""
    ids = np.zeros((len(seqs), L, 2), np.int64)
    mask = np.zeros((len(seqs), L - 1), np.float32)
    for u, seq in enumerate(seqs):
        seq = list(seq)[-L:]
        n = len(seq)
        own = set(seq)
        negs = []
        while len(negs) < n - 1:
            s = int(rng.integers(1, item_num + 1))
            if s not in own:
                negs.append(s)
        ids[u, L - n:, 0] = seq
        ids[u, L - n:L - 1, 1] = negs
        mask[u, L - n:] = 1.0
    return torch.from_numpy(ids.reshape(-1)), torch.from_numpy(mask)


def real_seqs():
    """tests/golden/real_data/amazon_users_head.tsv: item names renumbered 1.. in order of first appearance."""
    ids, out = {}, []
    with open(os.path.join(ROOT, 'tests', 'golden', 'real_data', 'amazon_users_head.tsv')) as f:
        for line in f:
            names = line.rstrip('\n').split('\t')[1].split(' ')
            out.append([ids.setdefault(nm, len(ids) + 1) for nm in names])
    return out


def list_stats(ids):
    """Lengths of the inverted index's lists (slots per distinct non-zero id) of one batch."""
    v = ids.numpy()
    _, c = np.unique(v[v > 0], return_counts=True)
    return dict(slots=int(v.size), distinct=int(c.size), longest_list=int(c.max()), median_list=float(np.median(c)),
                p99_list=float(np.quantile(c, 0.99)))


def make_batches(name, L, item_num, n_batches, rng):
    if name.startswith('real'):
        seqs = real_seqs()
        order = rng.permutation(len(seqs))
        return [batch_from_seqs([seqs[i] for i in order[k * B:(k + 1) * B]], L, item_num, rng) for k in range(n_batches)]
    return [batch_from_seqs([rng.integers(1, item_num + 1, L) for _ in range(B)], L, item_num, rng) for _ in range(n_batches)]


def _timed(fn, steps, warmup):
    """-> (ms per call, peak bytes allocated above the level before the first call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, torch.cuda.max_memory_allocated() - base


def head_compare(name, model, item_num, max_seq_len, steps, warmup, ce_dtype='fp32', skip_eager=False):
    """The cross-entropy head alone on B x max_seq_len rows against the model's table: the three fused launches beside eager fp32
    matmul + cross_entropy (forward and backward of both), same rows, same table, same targets."""
    from adapter4rec_amd import _lib as L
    R, N1 = B * max_seq_len, item_num + 1
    g = torch.Generator().manual_seed(1)
    table = model.id_embedding.weight.detach()
    prec = (torch.randn(R, E, generator=g) * E ** -0.25).cuda()
    tgt = torch.randint(1, N1, (R,), generator=g, dtype=torch.int32).cuda()
    mask = torch.ones(R, device='cuda')
    lse, s_tgt, lw = torch.empty(R, device='cuda'), torch.empty(R, device='cuda'), torch.empty(4, device='cuda')
    d_prec, d_table = torch.empty(R, E, device='cuda'), torch.zeros(N1, E, device='cuda')
    bf16 = ce_dtype == 'bf16'
    if bf16:
        ranges = L.score_ce_bf16_ranges(R, N1)
        ws = torch.empty(L.score_ce_bf16_ws_bytes(R, N1, E), dtype=torch.uint8, device='cuda')
        prec_b, table_b = torch.empty(R, E, dtype=torch.bfloat16, device='cuda'), torch.empty(N1, E, dtype=torch.bfloat16, device='cuda')
        head_fwd, head_bwd, a, b = L.score_ce_bf16_fwd, L.score_ce_bf16_bwd, prec_b, table_b
    else:
        ranges = L.score_ce_ranges(R, N1)
        ws = torch.empty(L.score_ce_ws_bytes(R, N1, E), dtype=torch.uint8, device='cuda')
        head_fwd, head_bwd, a, b = L.score_ce_fwd, L.score_ce_bwd, prec, table

    def cast():
        L.cast_bf16(table, table_b)
        L.cast_bf16(prec, prec_b)

    def fwd():
        head_fwd(a, b, tgt, mask, lse, s_tgt, lw, R, ws=ws)

    def rows():
        head_bwd(a, b, tgt, mask, lse, lw, 1.0, d_prec, None, R, ws=ws)

    def items():
        head_bwd(a, b, tgt, mask, lse, lw, 1.0, None, d_table, R)

    def fused():
        if bf16:
            cast()
        fwd()
        head_bwd(a, b, tgt, mask, lse, lw, 1.0, d_prec, d_table, R, ws=ws)

    pe, te, tl = prec.clone().requires_grad_(True), table.clone().requires_grad_(True), tgt.long() - 1

    def eager():
        pe.grad = te.grad = None
        loss = torch.nn.functional.cross_entropy(torch.matmul(pe, te[1:].T), tl)
        loss.backward()
        return loss

    fused_ms, fused_peak = _timed(fused, steps, warmup)
    eager_ms, eager_peak = (0.0, 0) if skip_eager else _timed(eager, steps, warmup)
    flop = 2.0 * R * item_num * E                          # one streamed product; forward 1, bwd_rows 2, bwd_items 2
    parts = {}
    for nm, fn, k in (('fwd', fwd, 1), ('bwd_rows', rows, 2), ('bwd_items', items, 2)):
        ms, _ = _timed(fn, steps, warmup)
        parts[nm + '_ms'] = round(ms, 4)
        parts[nm + '_mfma_fraction'] = round(k * flop / (ms * 1e-3) / FP32_MFMA_PEAK, 4)      # (of the fp32 peak under either --ce_dtype: one scale)
    if bf16:
        parts['cast_ms'] = round(_timed(cast, steps, warmup)[0], 4)
        parts['table_bf16_bytes'] = int(table_b.numel() * 2)
    return dict(config=name + '_ce_head', ce_dtype=ce_dtype, rows=R, item_num=item_num, embedding_dim=E, ranges=ranges, steps=steps, warmup=warmup,
                fused_ms=round(fused_ms, 4), eager_ms=round(eager_ms, 4), fused_peak_bytes=int(fused_peak), eager_peak_bytes=int(eager_peak),
                fused_ws_bytes=int(ws.numel()), logits_bytes=int(R * item_num * 4),
                fused_tflops_5_products=round(5 * flop / (fused_ms * 1e-3) / 1e12, 2), **parts,
                loss_fused=float(lw[0]), loss_eager=None if skip_eager else float(eager().detach()))


def run(name, max_seq_len, item_num, steps, warmup, loss_kind='bce', ce_dtype='fp32'):
    from adapter4rec_amd.cv import Model
    from adapter4rec_amd.cv.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdam
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    args = model_args(max_seq_len)
    args.loss = loss_kind
    args.ce_dtype = ce_dtype
    args.lr, args.fine_tune_lr, args.adapter_cv_lr, args.adapter_sasrec_lr = 1e-4, 1e-4, 1e-4, 1e-4
    model = Model(args, item_num, False).to('cuda')
    model.train()
    opt = FusedAdam(optimizer_groups(model, args))
    L = max_seq_len + 1
    batches = make_batches(name, L, item_num, 16, rng)
    stats = list_stats(batches[0][0])
    lens = [list_stats(b[0]) for b in batches]

    def step(i):
        items, mask = batches[i % len(batches)]
        opt.zero_grad()
        loss = model(items, mask, 0)
        loss.backward()
        opt.step()
        return loss

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = step(i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = dict(config=name, loss_kind=loss_kind, ce_dtype=ce_dtype, batch=B, embedding_dim=E, max_seq_len=max_seq_len, item_num=item_num, steps=steps, warmup=warmup,
                ms_per_step=round(dt * 1e3, 4), user_seq_per_s=round(B / dt, 1), loss=float(loss.detach()),
                longest_list_max=max(s['longest_list'] for s in lens), median_list_median=float(np.median([s['median_list'] for s in lens])),
                first_batch=stats)
    return out, model


CONFIGS = [('full_L10', 10, 14720), ('full_L20', 20, 14720), ('real_L20', 20, 14720), ('full_L20_500k', 20, 500000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--only', default=None)
    ap.add_argument('--loss', default='bce', choices=['bce', 'ce'])
    ap.add_argument('--ce_dtype', default='fp32', choices=['fp32', 'bf16'])
    ap.add_argument('--skip_eager', action='store_true')
    a = ap.parse_args()
    for name, msl, n in CONFIGS:
        if a.only and name != a.only:
            continue
        line, model = run(name, msl, n, a.steps, a.warmup, a.loss, a.ce_dtype)
        print(json.dumps(line), flush=True)
        if a.loss == 'ce':
            print(json.dumps(head_compare(name, model, n, msl, a.steps, a.warmup, a.ce_dtype, a.skip_eager)), flush=True)


if __name__ == '__main__':
    main()
