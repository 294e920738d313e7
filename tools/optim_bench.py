#!/usr/bin/env python
"""The optimizer step on one MI355X: a4r_adam_step, a4r_adamw_step without and with gradient-norm clipping (a4r_grad_sumsq + a4r_adamw_step), and
what a caller would write without the fused clip (torch.nn.utils.clip_grad_norm_ over the per-parameter views of the flat gradient buffer, then
a4r_adam_step) -- one JSON line per (size, variant).

    python tools/optim_bench.py [--iters N] [--only headline|bert_pretrain]

Sizes: the trainable parameters of bench.py's headline step (BERT-base + SASRec with Houlsby adapters) and of --workload bert_pretrain (full fine-
tuning), segment by segment in optimizer_groups' four lr groups, on flat fp32 buffers like the engine's.  Times are HIP-event means over N steps after
a warm-up; per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/optim_bench.py`."""
import argparse
import json
import os
import sys

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
    return a.elapsed_time(b) / iters * 1e3


def trainable_layout(workload):
    """[(numel, group)] of bench.py's model for `workload`, built on the host (only the shapes are used)."""
    import bench
    from adapter4rec_amd.inject import freeze_all, inject_adapters, optimizer_groups
    from adapter4rec_amd.model import BERT_BASE, BertBackbone, Model
    args = bench.make_args(32, 'bf16')
    torch.manual_seed(0)
    model = Model(args, 65536, True, BertBackbone(BERT_BASE))
    if workload == 'bert_pretrain':
        args.adapter_type, args.adding_adapter_to = 'none', 'None'
        for n, p in model.named_parameters():
            p.requires_grad = 'pooler' not in n
    else:
        freeze_all(model)
    model = inject_adapters(model, args)
    groups = optimizer_groups(model, args)
    return [(p.numel(), gi) for gi, g in enumerate(groups) for p in g['params']], [float(g['lr']) for g in groups]


def run(workload, iters):
    from adapter4rec_amd import _lib as L
    layout, lrs = trainable_layout(workload)
    n = sum(k for k, _ in layout)
    gen = torch.Generator(device=DEV).manual_seed(0)
    p = torch.randn(n, device=DEV, generator=gen) * 0.02
    g = torch.randn(n, device=DEV, generator=gen) * 1e-3
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ends = torch.tensor([k for k, _ in layout], dtype=torch.int64).cumsum(0).to(torch.int32)
    seg_end, seg_group = ends.to(DEV), torch.tensor([gi for _, gi in layout], dtype=torch.int32, device=DEV)
    glr = torch.tensor(lrs, device=DEV)
    gwd = torch.full((len(lrs),), 0.01, device=DEV)
    partials = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV)
    norm = torch.zeros((), device=DEV)
    views = [t for t in torch.split(g, [k for k, _ in layout])]
    params = [torch.nn.Parameter(torch.empty(t.shape, device=DEV)) for t in views]      # (only their .grad, the views, are read)
    for q, t in zip(params, views):
        q.grad = t
    max_norm = 0.5 * float(g.double().norm())           # clipping active
    step = [0]

    def adam():
        step[0] += 1
        L.adam_step(p, g, m, v, seg_end, seg_group, glr, step[0])

    def adamw():
        step[0] += 1
        L.adamw_step(p, g, m, v, seg_end, seg_group, glr, gwd, step[0], decoupled=True)

    def adamw_clip():
        step[0] += 1
        L.grad_sumsq(g, partials)
        L.adamw_step(p, g, m, v, seg_end, seg_group, glr, gwd, step[0], decoupled=True, partials=partials, max_norm=max_norm, norm_out=norm)

    g0 = g.clone()

    def eager_clip_adam():
        step[0] += 1
        torch.nn.utils.clip_grad_norm_(params, max_norm)   # rewrites g through the views
        L.adam_step(p, g, m, v, seg_end, seg_group, glr, step[0])

    out = {}
    for name, fn in (('adam_step', adam), ('adamw_step', adamw), ('adamw_step_clip', adamw_clip), ('eager_clip_grad_norm+adam_step', eager_clip_adam)):
        g.copy_(g0)
        out[name] = timed(fn, iters)
        print(json.dumps(dict(workload=workload, variant=name, n_params=n, n_segments=len(layout), iters=iters, us_per_step=round(out[name], 2))),
              flush=True)
    print(json.dumps(dict(workload=workload, n_params=n, clip_over_plain=round(out['adamw_step_clip'] / out['adam_step'], 3),
                          clip_minus_plain_us=round(out['adamw_step_clip'] - out['adam_step'], 2),
                          adamw_over_adam=round(out['adamw_step'] / out['adam_step'], 3),
                          eager_over_fused_clip=round(out['eager_clip_grad_norm+adam_step'] / out['adamw_step_clip'], 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--only', choices=['headline', 'bert_pretrain'])
    a = ap.parse_args()
    for wl in ('headline', 'bert_pretrain'):
        if a.only in (None, wl):
            run(wl, a.iters)


if __name__ == '__main__':
    main()
