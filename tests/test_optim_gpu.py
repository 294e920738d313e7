"""GPU: a4r_grad_sumsq / a4r_adamw_step (include/a4r.h) and FusedAdam / FusedAdamW with weight decay and gradient-norm clipping, against torch fp32
Adam / AdamW + torch.nn.utils.clip_grad_norm_, and against themselves across the quad / scalar paths.

Tolerances: the update matches torch within test_kernels_gpu.py::test_adam_matches_torch's rtol 1e-5 / atol 1e-7 (same arithmetic up to rounding;
torch forms the clipping norm in fp32, this library in fp64, so the coefficients may differ by an ulp).  The norm is held to 1 fp32 ulp of the fp64
norm of the same scaled fp32 gradients: every square is exact in fp64 and the fp64 summation error is below 2^-24 relative for n up to ~1e8, so
what remains is the single rounding to fp32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')


def rnd(n, seed, scale=1.0):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(DEV)


def segs(sizes, groups):
    seg_end = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=DEV)
    return seg_end, torch.tensor(groups, dtype=torch.int32, device=DEV)


SIZES, GROUPS = [1001, 63, 4097, 17, 2 ** 20 + 3, 5], [2, 0, 3, 1, 0, 3]      # odd segments straddling quads; n > 2^20: the quad kernel
LRS, WDS = [5e-4, 1e-3, 1.5e-3, 2e-3], [0.0, 0.01, 0.05, 0.2]


def torch_replay(p0, grads, decoupled, max_norm, grad_scale):
    """torch's own optimizer over the same segments and groups: returns (p, [norm per step] or None)."""
    params = [torch.nn.Parameter(x.clone()) for x in torch.split(p0.clone(), SIZES)]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{'params': [q], 'lr': LRS[g], 'weight_decay': WDS[g]} for q, g in zip(params, GROUPS)])
    norms = []
    for g in grads:
        for q, gg in zip(params, torch.split(g * grad_scale, SIZES)):
            q.grad = gg.clone()
        if max_norm is not None:
            norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm))
        opt.step()
    return torch.cat([q.detach() for q in params]), (norms or None)


def native(p0, grads, decoupled, max_norm, grad_scale, off=0):
    """a4r_grad_sumsq + a4r_adamw_step over buffers that start `off` floats into an allocation (off 1: misaligned -> the scalar kernels)."""
    from adapter4rec_amd import _lib as L
    n = p0.numel()
    seg_end, seg_group = segs(SIZES, GROUPS)
    glr, gwd = torch.tensor(LRS, device=DEV), torch.tensor(WDS, device=DEV)
    p, m, v, g = [torch.zeros(n + 4, device=DEV)[off:off + n] for _ in range(4)]
    p.copy_(p0)
    partials = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV)
    norms = []
    for step, gg in enumerate(grads, 1):
        g.copy_(gg)
        norm = None
        if max_norm is not None:
            norm = torch.zeros((), device=DEV)
            L.grad_sumsq(g, partials, grad_scale)
        L.adamw_step(p, g, m, v, seg_end, seg_group, glr, gwd, step, grad_scale=grad_scale, decoupled=decoupled,
                     partials=partials if norm is not None else None, max_norm=max_norm or 0.0, norm_out=norm)
        assert torch.equal(g, gg), 'the gradient buffer is not rewritten'
        norms.append(norm)
    return p.clone(), m.clone(), v.clone(), norms


def grads3(n):
    return [rnd(n, 80 + s) * (1.0 + 0.5 * s) for s in range(3)]


def fp64_norm(g, grad_scale):
    return float(torch.sqrt(((g * grad_scale).double() ** 2).sum()))


@pytest.mark.parametrize('decoupled', [0, 1])
@pytest.mark.parametrize('clip', ['off', 'inactive', 'active'])
def test_adamw_kernel_matches_torch(decoupled, clip):
    n = sum(SIZES)
    p0, grads, gs = rnd(n, 79), grads3(n), 0.5
    norm1 = fp64_norm(grads[0], gs)
    max_norm = dict(off=None, inactive=4.0 * norm1, active=0.3 * norm1)[clip]
    want, tnorms = torch_replay(p0, grads, decoupled, max_norm, gs)
    p, _, _, norms = native(p0, grads, decoupled, max_norm, gs)
    torch.testing.assert_close(p, want, rtol=1e-5, atol=1e-7)
    if max_norm is not None:
        for a, b in zip(norms, tnorms):
            torch.testing.assert_close(a, b.float(), rtol=1e-6, atol=0)      # (torch's own norm is an fp32 reduction)


def test_grad_norm_within_one_ulp_of_fp64():
    from adapter4rec_amd import _lib as L
    partials = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV)
    seg_end, seg_group = segs([1], [0])
    one = torch.ones(1, device=DEV)
    for n, scale, gs in ((1, 3.0, 1.0), (7, 1.0, 0.5), (262147, 1e-3, 1.0), (3 * 2 ** 20 + 5, 10.0, 0.25)):
        g = rnd(n, 90 + n, scale)
        L.grad_sumsq(g, partials, gs)
        # the norm itself comes out of a4r_adamw_step's prologue: one element run with a tiny max_norm
        norm = torch.zeros((), device=DEV)
        p, m, v = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        L.adamw_step(p, torch.zeros(1, device=DEV), m, v, seg_end, seg_group, one, one * 0, 1,
                     partials=partials, max_norm=1.0, norm_out=norm)
        ref = fp64_norm(g, gs)
        ulp = float(np.spacing(np.float32(ref)))
        assert abs(float(norm) - ref) <= ulp, (n, float(norm), ref)


@pytest.mark.parametrize('decoupled', [0, 1])
def test_quad_and_scalar_paths_bit_identical_and_repeatable(decoupled):
    n = sum(SIZES)
    p0, grads = rnd(n, 79), grads3(n)
    max_norm = 0.3 * fp64_norm(grads[0], 0.5)
    runs = [native(p0, grads, decoupled, max_norm, 0.5, off) for off in (0, 1, 0)]
    assert not torch.equal(runs[0][0], p0)
    for other in runs[1:]:
        for a, b in zip(runs[0][:3], other[:3]):
            assert torch.equal(a, b)
        for a, b in zip(runs[0][3], other[3]):
            assert torch.equal(a, b)
    # the partials themselves do not depend on the load path
    from adapter4rec_amd import _lib as L
    parts = []
    for off in (0, 1, 2, 3):
        g = torch.zeros(n + 4, device=DEV)[off:off + n]
        g.copy_(grads[1])
        pp = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV)
        L.grad_sumsq(g, pp, 0.5)
        parts.append(pp)
    for pp in parts[1:]:
        assert torch.equal(parts[0], pp)


@pytest.mark.parametrize('off', [0, 1])
def test_adamw_without_decay_or_clipping_equals_adam_step(off):
    from adapter4rec_amd import _lib as L
    n = sum(SIZES)
    seg_end, seg_group = segs(SIZES, GROUPS)
    glr, gwd = torch.tensor(LRS, device=DEV), torch.zeros(4, device=DEV)
    p0, grads = rnd(n, 79), grads3(n)
    outs = []
    for mode in ('adam', 0, 1):
        p, m, v, g = [torch.zeros(n + 4, device=DEV)[off:off + n] for _ in range(4)]
        p.copy_(p0)
        for step, gg in enumerate(grads, 1):
            g.copy_(gg)
            if mode == 'adam':
                L.adam_step(p, g, m, v, seg_end, seg_group, glr, step, grad_scale=0.5)
            else:
                L.adamw_step(p, g, m, v, seg_end, seg_group, glr, gwd, step, grad_scale=0.5, decoupled=mode)
        outs.append((p.clone(), m.clone(), v.clone()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_op_layer_fused_adamw_step_equals_binding():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import torch_ops
    ops = torch_ops.load()
    n = 5000
    seg_end, seg_group = segs([1000, 4000], [1, 0])
    glr, gwd = torch.tensor([1e-3, 2e-3], device=DEV), torch.tensor([0.05, 0.01], device=DEV)
    p0, g = rnd(n, 5), rnd(n, 6)
    max_norm = 0.5 * fp64_norm(g, 1.0)
    p1, m1, v1 = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    parts1, norm1 = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV), torch.zeros((), device=DEV)
    ops.fused_adamw_step(p1, g, m1, v1, seg_end, seg_group, glr, gwd, 1, decoupled=True, partials=parts1, max_norm=max_norm, norm_out=norm1)
    p2, m2, v2 = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    parts2, norm2 = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64, device=DEV), torch.zeros((), device=DEV)
    L.grad_sumsq(g, parts2)
    L.adamw_step(p2, g, m2, v2, seg_end, seg_group, glr, gwd, 1, decoupled=True, partials=parts2, max_norm=max_norm, norm_out=norm2)
    for a, b in ((p1, p2), (m1, m2), (v1, v2), (norm1, norm2), (parts1, parts2)):
        assert torch.equal(a, b)
    assert not torch.equal(p1, p0)
    schema = str(ops.fused_adamw_step.default._schema)
    assert 'Tensor(a!) p' in schema and 'Tensor(b!) m' in schema and 'Tensor(c!) v' in schema and 'Tensor(e!)? norm_out' in schema


def replay_steps(model, opt, ref_opt_cls, ref_kw, max_norm, batches):
    """Run `opt` over the batches; after each step replay torch's optimizer (+ clip_grad_norm_) on clones of the trainable parameters fed the same
    gradients, and compare.  Returns the largest |difference| seen."""
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    params = dict(model.named_parameters())
    clones = {n: torch.nn.Parameter(params[n].detach().clone()) for n in names}
    groups = [{'params': [clones[n] for n in names], **ref_kw}]
    ref = ref_opt_cls(groups)
    for batch in batches:
        opt.zero_grad()
        loss = model(*batch)
        loss.backward()
        for n in names:
            clones[n].grad = params[n].grad.detach().clone()
        opt.step()
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_([clones[n] for n in names], max_norm)
            assert float(tn) > max_norm, 'the clip is active'
            torch.testing.assert_close(opt.last_grad_norm, tn.float(), rtol=1e-6, atol=0)
        ref.step()
        for n in names:
            torch.testing.assert_close(params[n].detach(), clones[n].detach(), rtol=1e-5, atol=1e-7, msg=n)


def probe_norm(model, batch):
    """The total gradient norm of one step on `batch` (before any optimizer exists); the gradients are dropped again."""
    model(*batch).backward()
    ps = [p for p in model.parameters() if p.requires_grad]
    norm = float(torch.nn.utils.get_total_norm([p.grad for p in ps]))
    for p in ps:
        p.grad = None
    return norm


def test_engine_fused_adamw_clipped_three_steps_vs_torch():
    import test_engine_gpu as TG
    from adapter4rec_amd.optim import FusedAdamW
    root, args, sd, cfg, fx, items, mask = TG.build('houlsby', 'fp32')
    lr, batch = 1e-3, (items, mask, 0)
    max_norm = 0.5 * probe_norm(root, batch)
    opt = FusedAdamW([{'params': [p for p in root.parameters() if p.requires_grad], 'lr': lr}], weight_decay=0.05, max_grad_norm=max_norm)
    replay_steps(root, opt, torch.optim.AdamW, dict(lr=lr, weight_decay=0.05), max_norm, [batch] * 3)


def test_id_tower_fused_adam_coupled_decay_two_steps_vs_torch():
    import test_id_tower_cpu as CPU
    from adapter4rec_amd.optim import FusedAdam
    model, fx, _ = CPU.build('sasrec', compute_dtype='fp32')
    model = model.to(DEV)
    model.train()
    opt = FusedAdam([{'params': list(model.parameters()), 'lr': 1e-3}], weight_decay=0.05)
    batches = [(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0), (torch.from_numpy(fx['items2']), torch.from_numpy(fx['mask2']), 0)]
    replay_steps(model, opt, torch.optim.Adam, dict(lr=1e-3, weight_decay=0.05), None, batches)
