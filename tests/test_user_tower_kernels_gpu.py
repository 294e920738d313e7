"""The user tower's hand-written kernels against fp64 references at their shape edges:
  * a4r_sasrec_block_fwd / _bwd (csrc/a4r_sasrec.hip) against tests/sasrec_ref.py, on the cases tests/test_sasrec_ref_cpu.py proves sound
    (scores below 32 so that the exact-mask reference describes the kernel, no user near a ReLU kink);
  * a4r_score_bce_fwd / _bwd, a4r_take_inputs, a4r_emb_grad_add_inputs (csrc/a4r_head.hip) against an fp64 restatement in this file.
The bounds are the ones tests/test_kernels_gpu.py already holds these kernels to: y 5e-5, dx 1e-4 (atol = rtol), each weight gradient
1e-4 * max |ref| + 1e-6 (rtol 1e-4); head scores 2e-4, head gradients 1e-6 absolute (rtol 2e-4), loss 1e-5.

Measured maximum errors against the fp64 reference on an MI355X, next to the error of a plain fp32 evaluation of the same reference on the
CPU ("fp32 CPU"; printed by tests/test_sasrec_ref_cpu.py).  gw = worst adapter / LN3 gradient error over max |gradient|.  Where a case runs in
several tests (accumulation, null sinks) the kernel column is the worst of them.

    case                       kernel y   dx        gw       | fp32 CPU y  dx        gw
    (bound)                    5e-5       1e-4      1e-4     |
    T1                         1.3e-06    1.2e-06   4.7e-07  | 9.0e-07     1.2e-06   6.4e-07
    T2                         1.2e-06    2.8e-06   3.9e-07  | 1.2e-06     2.5e-06   4.7e-07
    T15                        1.4e-06    3.5e-06   5.3e-07  | 1.8e-06     4.5e-06   5.5e-07
    T16                        1.7e-06    3.3e-06   4.2e-07  | 1.9e-06     3.4e-06   5.9e-07
    T17                        1.4e-06    4.7e-06   4.6e-07  | 1.6e-06     4.2e-06   4.1e-07
    T31                        1.7e-06    3.8e-06   5.4e-07  | 1.5e-06     4.4e-06   6.6e-07
    T32                        1.9e-06    5.0e-06   4.0e-07  | 1.5e-06     4.2e-06   4.5e-07
    T32_d1_ldwu16              1.5e-06    3.0e-06   1.5e-06  | 1.3e-06     2.9e-06   1.7e-06
    T32_d1_ldwu64              1.4e-06    2.9e-06   1.0e-05  | 2.0e-06     4.1e-06   1.0e-05
    T32_d15_ldwu16             1.8e-06    3.4e-06   4.1e-07  | 1.9e-06     5.1e-06   6.0e-07
    T32_d15_ldwu64             1.8e-06    4.5e-06   5.0e-07  | 1.8e-06     4.3e-06   5.6e-07
    T32_d16_ldwu16             1.7e-06    5.2e-06   6.0e-07  | 2.1e-06     4.7e-06   6.7e-07
    T32_d16_ldwu64             1.4e-06    4.5e-06   6.3e-07  | 1.9e-06     4.2e-06   6.5e-07
    T32_d17_ldwu32             1.6e-06    5.5e-06   5.9e-07  | 1.5e-06     4.0e-06   5.8e-07
    T32_d17_ldwu64             1.7e-06    5.1e-06   5.1e-07  | 1.7e-06     5.0e-06   6.7e-07
    T32_d32_ldwu32             2.4e-06    6.9e-06   5.6e-07  | 2.4e-06     7.4e-06   5.7e-07
    T32_d32_ldwu64             2.4e-06    6.3e-06   5.7e-07  | 2.0e-06     5.5e-06   6.2e-07
    T17_d1_ldwu16              1.5e-06    2.6e-06   6.2e-07  | 2.1e-06     3.0e-06   1.1e-06
    T17_d1_ldwu64              1.5e-06    5.1e-06   8.6e-07  | 2.0e-06     4.4e-06   8.3e-07
    T17_d15_ldwu16             1.6e-06    3.0e-06   5.1e-07  | 1.5e-06     6.4e-06   5.6e-07
    T17_d15_ldwu64             2.0e-06    3.3e-06   4.8e-07  | 1.5e-06     3.5e-06   6.4e-07
    T17_d16_ldwu16             1.6e-06    3.8e-06   5.9e-07  | 1.7e-06     3.8e-06   6.6e-07
    T17_d16_ldwu64             1.6e-06    5.2e-06   6.7e-07  | 1.8e-06     4.4e-06   6.8e-07
    T17_d17_ldwu32             1.8e-06    4.4e-06   7.4e-07  | 1.5e-06     3.1e-06   4.2e-07
    T17_d17_ldwu64             1.5e-06    3.2e-06   4.5e-07  | 1.4e-06     4.1e-06   4.1e-07
    T17_d32_ldwu32             1.6e-06    5.0e-06   5.6e-07  | 1.6e-06     5.2e-06   6.2e-07
    T17_d32_ldwu64             1.8e-06    5.0e-06   7.2e-07  | 1.8e-06     5.8e-06   8.0e-07
    mode0_inner1_act0          1.8e-06    4.2e-06   6.0e-07  | 1.7e-06     4.1e-06   5.8e-07
    mode0_inner1_act1          1.8e-06    5.2e-06   5.2e-07  | 1.9e-06     4.8e-06   5.8e-07
    mode0_inner1_act2          1.7e-06    5.9e-06   7.7e-07  | 1.8e-06     5.3e-06   6.6e-07
    mode0_inner1_act3          1.9e-06    4.2e-06   6.9e-07  | 1.9e-06     4.6e-06   9.4e-07
    mode0_inner1_act4          1.6e-06    5.7e-06   5.4e-07  | 1.5e-06     4.0e-06   7.0e-07
    mode0_inner0_act0          1.8e-06    4.3e-06   5.6e-07  | 2.2e-06     3.8e-06   6.2e-07
    mode0_inner0_act1          1.5e-06    3.4e-06   4.4e-07  | 1.4e-06     4.2e-06   8.6e-07
    mode0_inner0_act2          1.6e-06    5.1e-06   7.5e-07  | 1.7e-06     5.2e-06   8.5e-07
    mode0_inner0_act3          2.3e-06    4.9e-06   6.8e-07  | 1.7e-06     5.1e-06   6.9e-07
    mode0_inner0_act4          1.5e-06    4.4e-06   4.7e-07  | 1.3e-06     5.5e-06   5.5e-07
    mode1_inner0_act0          1.4e-06    3.3e-06   4.8e-07  | 2.0e-06     3.5e-06   6.0e-07
    mode1_inner0_act1          1.3e-06    3.4e-06   4.2e-07  | 1.6e-06     3.9e-06   5.9e-07
    mode1_inner0_act2          1.4e-06    3.2e-06   6.7e-07  | 1.3e-06     4.1e-06   5.3e-07
    mode1_inner0_act3          1.4e-06    3.9e-06   4.8e-07  | 1.5e-06     4.6e-06   5.9e-07
    mode1_inner0_act4          1.6e-06    3.0e-06   2.7e-07  | 1.4e-06     2.6e-06   4.7e-07
    big_T32                    2.7e-06    7.2e-06   1.2e-06  | 2.4e-06     8.1e-06   6.3e-07
    big_T17                    2.4e-06    8.3e-06   8.8e-07  | 2.3e-06     8.7e-06   6.1e-07
    drop_T17_mode0_both        2.3e-06    4.4e-06   5.9e-07  | 2.3e-06     7.1e-06   6.0e-07
    drop_T17_mode0_attn        1.5e-06    4.1e-06   5.5e-07  | 1.5e-06     4.1e-06   7.1e-07
    drop_T17_mode0_hidden      1.7e-06    4.4e-06   5.1e-07  | 1.5e-06     4.1e-06   5.5e-07
    drop_T17_mode1_both        1.8e-06    2.6e-06   3.4e-07  | 1.5e-06     2.5e-06   4.4e-07
    drop_T17_mode1_attn        1.9e-06    3.6e-06   3.0e-07  | 1.3e-06     3.8e-06   3.5e-07
    drop_T17_mode1_hidden      1.6e-06    2.7e-06   3.9e-07  | 1.5e-06     2.8e-06   4.2e-07
    drop_T32_mode0_both        1.9e-06    4.0e-06   4.4e-07  | 1.6e-06     4.8e-06   5.5e-07
    drop_T32_mode0_attn        1.6e-06    4.9e-06   4.4e-07  | 1.6e-06     4.0e-06   8.3e-07
    drop_T32_mode0_hidden      2.7e-06    4.4e-06   8.6e-07  | 2.0e-06     3.8e-06   6.8e-07
    drop_T32_mode1_both        1.9e-06    3.0e-06   3.2e-07  | 1.4e-06     3.5e-06   4.4e-07
    drop_T32_mode1_attn        1.5e-06    4.3e-06   4.3e-07  | 1.5e-06     3.8e-06   5.5e-07
    drop_T32_mode1_hidden      2.2e-06    4.1e-06   3.0e-07  | 1.5e-06     3.7e-06   5.0e-07

Scoring head (kernel only; bounds: scores 2e-4, loss 1e-5, gradients 1e-6 + 2e-4 |ref|; gradients with loss_scale 0.37, then 0.37 x 2.5):
    B=6 L=21 E=64 cpc=0 pos=2.58e-07 loss=8.23e-08 d_prec=7.27e-10 d_emb=6.40e-10 d_prec=2.54e-09 d_emb=2.10e-09
    B=6 L=21 E=64 cpc=1 pos=2.58e-07 loss=4.63e-08 d_prec=4.38e-09 d_emb=4.60e-09 d_prec=9.87e-09 d_emb=6.54e-09
    B=3 L=2 E=64 cpc=0 pos=1.17e-07 loss=5.68e-08 d_prec=6.83e-09 d_emb=8.24e-09 d_prec=2.19e-08 d_emb=1.97e-08
    B=3 L=2 E=64 cpc=1 pos=1.17e-07 loss=2.50e-08 d_prec=4.75e-09 d_emb=4.87e-09 d_prec=1.27e-08 d_emb=1.62e-08
    B=5 L=33 E=256 cpc=0 pos=2.18e-07 loss=2.62e-07 d_prec=4.20e-10 d_emb=2.77e-10 d_prec=8.59e-10 d_emb=6.80e-10
    B=5 L=33 E=256 cpc=1 pos=2.18e-07 loss=7.38e-08 d_prec=5.22e-09 d_emb=3.25e-09 d_prec=9.50e-09 d_emb=6.37e-09
    B=7 L=9 E=100 cpc=0 pos=1.85e-07 loss=1.94e-07 d_prec=1.35e-09 d_emb=1.27e-09 d_prec=3.35e-09 d_emb=2.55e-09
    B=7 L=9 E=100 cpc=1 pos=1.85e-07 loss=4.17e-08 d_prec=4.83e-09 d_emb=5.07e-09 d_prec=1.22e-08 d_emb=1.02e-08
    B=260 L=21 E=64 cpc=0 pos=3.64e-07 loss=1.24e-06 d_prec=2.38e-11 d_emb=2.13e-11 d_prec=7.47e-11 d_emb=7.04e-11
    B=260 L=21 E=64 cpc=1 pos=3.64e-07 loss=1.29e-09 d_prec=2.07e-10 d_emb=1.90e-10 d_prec=6.02e-10 d_emb=3.99e-10
"""
import pytest
import torch

import sasrec_ref as R

pytestmark = pytest.mark.gpu

Y_TOL, DX_TOL, G_TOL = 5e-5, 1e-4, 1e-4


def dev():
    return torch.device('cuda:0')


def _worst(what, got, ref, atol, rtol):
    """max |got - ref| after asserting |got - ref| <= atol + rtol |ref| elementwise (fp64 on the host)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), (f'{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.3e} '
                           f'(ref max {float(ref.abs().max()):.3e}) first bad idx {bad.nonzero()[0].tolist()}')
    return float(err.max())


# ------------------------------------------------------------------ the block
def _sink_shapes(c):
    """Gradient sinks with the case's leading dimensions, one spare row behind the matrices: everything outside the [d, 64] / [64, d] / [d]
    corners must come back untouched."""
    d, s = c.d, c.spec
    return {'wd': (d + 1, s.get('ldg_d', 64)), 'wu': (65, s.get('ldg_u', 64)), 'bd': (R.dpe_of(d),), 'bu': (64,), 'ln3_g': (64,), 'ln3_b': (64,)}


def _device_desc(c, prefill=None, null=()):
    """The case's descriptor on the device.  prefill: None (zero sinks) or a seed (sinks pre-filled with random values in [1, 2))."""
    desc = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in c.desc.items()}
    shapes = _sink_shapes(c)
    g = torch.Generator().manual_seed(prefill or 0)
    names = R.ADAPTER_GRADS + (('ln3_g', 'ln3_b') if c.spec.get('mode', 0) == 1 else ())
    for k in names:
        shp = shapes[k if k.startswith('ln3') else k[:2]]
        t = torch.zeros(shp) if prefill is None else 1 + torch.rand(shp, generator=g)
        desc['g_' + k] = None if k in null else t.to(dev())
    return desc


def _corner(k, t, d):
    """The part of sink k that holds the gradient."""
    return t[:d, :64] if k.startswith('wd') else t[:64, :d] if k.startswith('wu') else t[:d] if k.startswith('bd') else t


def _check_sinks(c, desc, before, times=1, skip=()):
    """Every non-null sink == before + times * reference gradient inside its corner (the gradient bound, on the added amount) and
    bit-identical to `before` outside.  Returns the worst error relative to max |ref|."""
    worst = 0.0
    live = R.grad_names(c.spec.get('mode', 0))
    for k, b in before.items():
        got = desc['g_' + k]
        if got is None or k in skip:
            continue
        got, b = got.cpu(), b.cpu()
        if k not in live:                                           # mode 1: adapter 1 does not exist
            assert torch.equal(got, b), f'{c.name}: g_{k} was written'
            continue
        ref = c.ref.grads[k] * times
        m = float(ref.abs().max())
        added = _corner(k, got, c.d).double() - _corner(k, b, c.d).double()
        worst = max(worst, _worst(f'{c.name} g_{k}', added, ref, G_TOL * m + 1e-6, G_TOL) / max(m, 1e-30))
        outside = torch.ones_like(got, dtype=torch.bool)
        _corner(k, outside, c.d)[...] = False
        assert torch.equal(got[outside], b[outside]), f'{c.name}: g_{k} was written outside its corner'
    return worst


def _run_block(c, prefill=None, null=(), times=1, train=False):
    """Forward and `times` backward launches of case c against its fp64 reference; prints the case's figures."""
    from adapter4rec_amd import _lib as L
    desc = _device_desc(c, prefill, null)
    before = {k[2:]: v.clone() for k, v in desc.items() if k.startswith('g_') and v is not None}
    x, mask, dy = c.x.to(dev()), c.mask.to(dev()), c.dy.to(dev())
    y, dx = torch.full_like(x, float('nan')), torch.full_like(x, float('nan'))
    L.sasrec_block(desc, x, mask, y, c.B, c.T, train)
    for _ in range(times):
        L.sasrec_block(desc, x, mask, dx, c.B, c.T, train, dy=dy)
    torch.cuda.synchronize()
    ey = _worst(f'{c.name} y', y, c.ref.y, Y_TOL, Y_TOL)
    ex = _worst(f'{c.name} dx', dx, c.ref.dx, DX_TOL, DX_TOL)
    eg = _check_sinks(c, desc, before, times)
    print(f'GPU {c.name} y={ey:.2e} dx={ex:.2e} gw={eg:.2e}')
    return desc, y, dx


@pytest.mark.parametrize('name', R.names('T'))
def test_block_sequence_lengths(name):
    """T on every side of the two 16-row tiles; users with 0, 1, T - 1 and T padded positions."""
    _run_block(R.reference(name))


@pytest.mark.parametrize('name', R.names('d'))
def test_block_adapter_widths_and_leading_dimensions(name):
    """d on every side of the 16-column tile with ldwu = dpe and 64, compact g_wu (ld = d), g_wd with ld 68; sinks pre-filled with a
    pattern that must survive outside the [d, 64] / [64, d] corners; non-zero values in the padding of Wd / bd / Wu."""
    _run_block(R.reference(name), prefill=11)


@pytest.mark.parametrize('name', R.names('act'))
def test_block_modes_and_activations(name):
    _run_block(R.reference(name))


@pytest.mark.parametrize('name', ['T17', 'T32_d17_ldwu32', 'mode1_inner0_act3'])
def test_block_gradients_accumulate(name):
    """g_* += : random sinks, two backward launches -> prefill + 2 * gradient (fp32 atomics: the gradient bound, not bitwise)."""
    _run_block(R.reference(name), prefill=23, times=2)


@pytest.mark.parametrize('name', ['T17', 'mode1_inner0_act1'])
def test_block_null_sinks(name):
    """"any may be null": without any sink dx is still right; without the Wu sinks the remaining gradients are."""
    c = R.reference(name)
    _run_block(c, null=R.ADAPTER_GRADS + ('ln3_g', 'ln3_b'))
    _run_block(c, null=('wu1', 'wu2'))


@pytest.mark.parametrize('name', R.names('big'))
def test_block_many_users(name):
    """600 workgroups (more than two per CU): the launch wraps.  Users near a ReLU kink have dy = 0 and must get dx == 0 exactly; a
    user's forward output does not depend on its neighbours or its workgroup index."""
    from adapter4rec_amd import _lib as L
    c = R.reference(name)
    desc, y, dx = _run_block(c)
    B, T = c.B, c.T
    assert c.kink.any() and float(dx.view(B, T, 64)[c.kink.to(dev())].abs().max()) == 0.0
    x, mask = c.x.to(dev()), c.mask.to(dev())
    for u in (0, B // 2 - 1, B - 1):
        y1 = torch.full((T, 64), float('nan'), device=dev())
        L.sasrec_block(desc, x[u * T:(u + 1) * T], mask[u:u + 1], y1, 1, T, False)
        assert torch.equal(y1, y[u * T:(u + 1) * T]), f'{name}: user {u} differs from a launch of that user alone'


@pytest.mark.parametrize('name', R.names('drop'))
def test_block_dropout_identical_masks(name):
    """train = 1 against the fp64 reference multiplied by the very masks the kernel draws (oracle/dropout_masks.py)."""
    c = R.reference(name)
    assert any(float((m == 0).float().mean()) > 0.05 for m in c.masks.values())
    _run_block(c, train=True)


def _reject_cases():
    return [('T = 0', dict(T=0), {}), ('T = 33', dict(T=33), {}), ('d = 0', {}, dict(d=0)), ('dpe > ldwu', {}, dict(d=17, ldwu=20)),
            ('ldwu % 4', {}, dict(ldwu=18)), ('E = 32', {}, dict(E=32)), ('mode = 2', {}, dict(mode=2)), ('mode 1 without ln3_g', {}, dict(mode=1, ln3_g=None)),
            ('drop_attn = 1', dict(train=True), dict(drop_attn=1.0)), ('x 4 bytes into a buffer', dict(shift=True), {}),
            ('ldg_d = 32', dict(bwd=True), dict(ldg_d=32)), ('ldg_u = d - 1', dict(bwd=True), dict(ldg_u=15))]


@pytest.mark.parametrize('what,call,over', _reject_cases(), ids=[w for w, _, _ in _reject_cases()])
def test_block_rejects(what, call, over):
    """Argument checks of fill() and the entry points: the library's invalid-argument status and nothing launched (the output keeps its
    fill).  One field is wrong per case (d = 16, T = 17 otherwise); every buffer would be large enough had the call been accepted."""
    from adapter4rec_amd import _lib as L
    c = R.reference('T17')
    B, T = c.B, call.get('T', c.T)
    desc = _device_desc(c)
    z = lambda *s: torch.zeros(*s, device=dev())
    for k in ('1', '2'):                                            # 64-wide adapter operands and sinks: room for any d / ld a case asks for
        desc.update({'wd' + k: z(64, 64), 'bd' + k: z(64), 'wu' + k: z(64, 64), 'g_wd' + k: z(64, 68), 'g_bd' + k: z(64), 'g_wu' + k: z(64, 64)})
    desc.update(ln3_g=z(64), ln3_b=z(64), g_ln3_g=None, g_ln3_b=None)
    desc.update(over)
    rows = B * 33
    buf = z(rows * 64 + 4)
    x = buf[1:1 + rows * 64].view(rows, 64) if call.get('shift') else buf[:rows * 64].view(rows, 64)
    mask, out = torch.ones(B, 33, device=dev()), torch.full((rows, 64), 7.0, device=dev())
    with pytest.raises(RuntimeError, match=r'status -1 \(invalid argument\)'):
        L.sasrec_block(desc, x, mask, out, B, T, call.get('train', False), dy=z(rows, 64) if call.get('bwd') else None)
    torch.cuda.synchronize()
    assert float((out - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------ the scoring head
def _head_case(B, L, E, seed):
    """prec / emb scaled so that the scores have unit variance (E ** -0.25 each), as in a trained model: the loss bound (1e-5 absolute) is
    an fp32 statement about a loss of order 1.  Left padding per user, user 1 fully padded."""
    g = torch.Generator().manual_seed(seed)
    emb, prec = torch.randn(B, L, 2, E, generator=g) * E ** -0.25, torch.randn(B, L - 1, E, generator=g) * E ** -0.25
    mask = torch.ones(B, L - 1)
    for b in range(B):
        mask[b, :(L - 1 if b == 1 else (3 * b) % (L - 1))] = 0
    return emb, prec, mask


def _head_ref(emb, prec, mask, cpc):
    """fp64: pos[b, t] = prec[b, t] . emb[b, t + 1, 0], neg[b, t] = prec[b, t] . emb[b, t, 1]; loss = mean over the valid (b, t) of
    softplus(-pos) + softplus(neg); valid = log_mask != 0, or (CPC) the last position of every user."""
    e, p = emb.double().requires_grad_(True), prec.double().requires_grad_(True)
    pos, neg = (p * e[:, 1:, 0]).sum(-1), (p * e[:, :-1, 1]).sum(-1)
    valid = torch.zeros_like(mask, dtype=torch.bool)
    if cpc:
        valid[:, -1] = True
    else:
        valid = mask != 0
    sp = torch.nn.functional.softplus
    loss = (sp(-pos[valid]) + sp(neg[valid])).mean()
    d_emb, d_prec = torch.autograd.grad(loss, [e, p])
    return pos.detach(), neg.detach(), float(loss.detach()), d_prec, d_emb, valid


HEAD_SHAPES = [(6, 21, 64), (3, 2, 64), (5, 33, 256), (7, 9, 100), (260, 21, 64)]


@pytest.mark.parametrize('cpc', [False, True])
@pytest.mark.parametrize('B,L,E', HEAD_SHAPES)
def test_head_vs_fp64(B, L, E, cpc):
    """T = 1, E = 256, E not a multiple of 64, and 5 200 / 5 460 rows (past the 4 096-row grid: the grid-stride loops run);
    loss_scale with and without a device-side factor; every output element overwritten; exact zeros where no gradient flows."""
    from adapter4rec_amd import _lib as Lb
    emb, prec, mask = _head_case(B, L, E, seed=300 + B + L + E)
    pos_r, neg_r, loss_r, dprec_r, demb_r, valid = _head_ref(emb, prec, mask, cpc)
    assert valid.any() and not (mask[1] != 0).any() and (mask[0] != 0).all()           # a fully padded user next to a full one
    e, p, m = emb.to(dev()), prec.to(dev()), mask.to(dev())
    nan = float('nan')
    pos, neg = torch.full((B, L - 1), nan, device=dev()), torch.full((B, L - 1), nan, device=dev())
    ws = torch.zeros(4, device=dev())
    Lb.score_bce_fwd(e, p, m, pos, neg, ws, B, L, E, cpc)
    e_pos = _worst('pos', pos, pos_r, 2e-4, 2e-4)
    e_neg = _worst('neg', neg, neg_r, 2e-4, 2e-4)
    e_loss = abs(float(ws[0]) - loss_r)
    assert float(ws[2]) == float(valid.sum())
    fig = f'GPU head B={B} L={L} E={E} cpc={int(cpc)} pos={max(e_pos, e_neg):.2e} loss={e_loss:.2e}'
    assert e_loss < 1e-5, fig
    for scale_dev in (None, torch.tensor([2.5], device=dev())):
        s = 0.37 * (2.5 if scale_dev is not None else 1.0)
        d_prec, d_emb = torch.full_like(p, nan), torch.full_like(e, nan)
        Lb.score_bce_bwd(e, p, m, pos, neg, ws, 0.37, d_prec, d_emb, B, L, E, cpc, scale_dev=scale_dev)
        e_dp = _worst('d_prec', d_prec, dprec_r * s, 1e-6, 2e-4)           # (NaN anywhere = an element the backward did not write)
        e_de = _worst('d_emb', d_emb, demb_r * s, 1e-6, 2e-4)
        fig += f' d_prec={e_dp:.2e} d_emb={e_de:.2e}'
        inv = ~valid.to(dev())
        amax = lambda t: float(t.abs().max()) if t.numel() else 0.0
        assert amax(d_emb[:, 0, 0]) == 0.0 and amax(d_emb[:, L - 1, 1]) == 0.0
        assert amax(d_emb[:, 1:, 0][inv]) == 0.0 and amax(d_emb[:, :-1, 1][inv]) == 0.0 and amax(d_prec[inv]) == 0.0
        assert float(d_emb.abs().max()) > 0.0
    print(fig)


@pytest.mark.parametrize('B,L,E', [(5, 4, 64), (7, 12, 100), (37, 30, 256)])
def test_head_input_pieces_with_padded_rows(B, L, E):
    """a4r_take_inputs / a4r_emb_grad_add_inputs with ldo = ldi = E + 8 and 15 / 77 / 1 073 rows (37 x 29 x 256 elements: past the
    1 024 x 256 grid, the stride loop runs): exact copy, one fp32 addition per element, nothing else touched."""
    from adapter4rec_amd import _lib as Lb
    rows, ld = B * (L - 1), E + 8
    g = torch.Generator().manual_seed(500 + B)
    emb = torch.randn(B, L, 2, E, generator=g).to(dev())
    out = torch.full((rows + 3, ld), 5.0, device=dev())
    Lb.take_inputs(emb, out[:, :E], B, L, E)
    want = torch.full((rows + 3, ld), 5.0, device=dev())
    want[:rows, :E] = emb[:, :-1, 0].reshape(rows, E)
    assert torch.equal(out, want)
    d_in = torch.randn(rows + 3, ld, generator=g).to(dev())
    d_emb = torch.randn(B, L, 2, E, generator=g).to(dev())
    want = d_emb.clone()
    want[:, :-1, 0] += d_in[:rows, :E].reshape(B, L - 1, E)
    Lb.emb_grad_add_inputs(d_in[:, :E], d_emb, B, L, E)
    assert torch.equal(d_emb, want)
