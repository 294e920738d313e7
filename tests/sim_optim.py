"""TEST-ONLY torch restatement of a4r_grad_sumsq / a4r_adamw_step (include/a4r.h) on the CPU, for the host logic of FusedAdam / FusedAdamW.
Tests monkeypatch these two into tests/sim_lib.py next to its adam_step (`install(monkeypatch)`).  The partials hold the header's fixed element
shares (thread t of A4R_GRAD_NORM_PARTS x 256 owns quads t, t + T, ...), so their sum is the header's sum up to fp64 rounding."""
import math

import torch

GRAD_NORM_PARTS = 1024


def grad_sumsq(g, partials, grad_scale=1.0):
    x = (g.float() * grad_scale).double() ** 2
    T = GRAD_NORM_PARTS * 256
    nq = (x.numel() + 3) // 4
    q = torch.zeros(nq * 4, dtype=torch.float64)
    q[:x.numel()] = x
    per_quad = q.view(nq, 4).sum(1)
    thread = torch.arange(nq) % T
    partials.zero_()
    partials.index_add_(0, thread // 256, per_quad)


def adamw_step(p, g, m, v, seg_end, seg_group, group_lr, group_wd, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, decoupled=True,
               partials=None, max_norm=0.0, norm_out=None):
    idx = torch.arange(p.numel())
    seg = torch.searchsorted(seg_end.long(), idx, right=True).clamp(max=seg_end.numel() - 1)
    grp = seg_group.long()[seg]
    lr, wd = group_lr[grp], group_wd[grp]
    gi = g * grad_scale
    if partials is not None:
        norm = torch.sqrt(partials.sum()).float()
        if norm_out is not None:
            norm_out.copy_(norm)
        c = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
        coef = torch.where(c > 1, torch.ones_like(c), c)
        gi = gi * coef
    if decoupled:
        p.mul_(1 - lr * wd)
    else:
        gi = gi + wd * p
    m.mul_(beta1).add_(gi, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gi, gi, value=1 - beta2)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p.sub_((lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps))


def install(monkeypatch):
    import sim_lib
    monkeypatch.setattr(sim_lib, 'GRAD_NORM_PARTS', GRAD_NORM_PARTS, raising=False)
    monkeypatch.setattr(sim_lib, 'grad_sumsq', grad_sumsq, raising=False)
    monkeypatch.setattr(sim_lib, 'adamw_step', adamw_step, raising=False)
