"""The cases of tests/test_user_tower_kernels_gpu.py, proved sound without a GPU.  For every case of sasrec_ref.CASES:
  (a) the new reference evaluated in fp32 agrees with sim_lib.sasrec_block (fp32, validated by the CPU engine suite) within the block's
      fp32 bounds, and with its own fp64 evaluation within the same bounds (the figure the GPU file's table quotes as "fp32 CPU");
  (b) max |scaled score| < 32: fp32 `s + mask_neg` is exactly mask_neg, so the exact-mask reference describes the kernel;
  (c) no user of a small case is near a ReLU kink; at most 10 % of a many-user case's users are, and those have dy = 0.
"""
import pytest
import torch

import sasrec_ref as R
import sim_lib

Y_TOL, DX_TOL, G_TOL = 5e-5, 1e-4, 1e-4          # the block's bounds in tests/test_kernels_gpu.py: y, dx (atol = rtol), gradients (x max |ref| + 1e-6)


def _worst(got, ref, atol, rtol):
    err = (got.double() - ref.double()).abs()
    return float(err.max()), float((err / (atol + rtol * ref.double().abs())).max())


def _compare(what, a, a_grads, b, b_grads):
    """y / dx / gradients of evaluation a against b: (max err y, max err dx, max err / max |ref| over the gradients); asserts the bounds."""
    ey, ry = _worst(a[0], b[0], Y_TOL, Y_TOL)
    ex, rx = _worst(a[1], b[1], DX_TOL, DX_TOL)
    eg, rg = 0.0, 0.0
    for k, ref in b_grads.items():
        m = float(ref.abs().max())
        e, r = _worst(a_grads[k], ref, G_TOL * m + 1e-6, G_TOL)
        eg, rg = max(eg, e / max(m, 1e-30)), max(rg, r)
    print(f'{what} y={ey:.2e} dx={ex:.2e} gw={eg:.2e}')
    assert ry <= 1 and rx <= 1 and rg <= 1, (what, ry, rx, rg)
    return ey, ex, eg


@pytest.mark.parametrize('name', list(R.CASES))
def test_case_is_sound(name):
    c = R.reference(name)
    B, T, d, mode = c.B, c.T, c.d, c.spec.get('mode', 0)
    # (b)
    assert c.ref.smax < R.SMAX, c.ref.smax
    # (c)
    share = float(c.kink.float().mean())
    if B <= 8:
        assert not c.kink.any(), f'{name}: users {c.kink.nonzero().flatten().tolist()} are near a kink: pick another seed (sasrec_ref.SEEDS)'
    else:
        assert share <= R.KINK_CAP, (name, share)
        assert c.kink.any(), 'a many-user case without a user near a kink would leave the dy = 0 rule unexercised'
        assert float(c.dy.view(B, T, -1)[c.kink].abs().max()) == 0.0
        assert float(c.ref.dx.view(B, T, -1)[c.kink].abs().max()) == 0.0          # such a user contributes exactly nothing
    # the kink statistic must look at what it claims to: every kinked site present, rows < T of every user
    want = {'ffn'} | ({'ad2'} | ({'ad1'} if mode == 0 else set()) if c.spec.get('act', 1) in (1, 4) else set())
    assert set(c.ref.pre) == want and c.ref.pre['ffn'].shape == (B, T, R.F)
    # (a) fp32 evaluation of the new reference against its fp64 evaluation (with the case's masks) ...
    f32 = R.block_ref(c.desc, c.x, c.mask, T, dy=c.dy, masks=c.masks, dtype=torch.float32)
    _compare(f'FP32 {name}', (f32.y, f32.dx), f32.grads, (c.ref.y, c.ref.dx), c.ref.grads)
    # ... and against sim_lib's restatement, dropout off (sim_lib has none)
    if c.masks is not None:
        f32 = R.block_ref(c.desc, c.x, c.mask, T, dy=c.dy, dtype=torch.float32)
    sd = dict(c.desc, drop_attn=0.0, drop_hidden=0.0)
    for k in R.grad_names(mode):
        sd['g_' + k] = torch.zeros_like(f32.grads[k])
    y, dx = torch.zeros(B * T, 64), torch.zeros(B * T, 64)
    sim_lib.sasrec_block(sd, c.x, c.mask, y, B, T, False)
    sim_lib.sasrec_block(sd, c.x, c.mask, dx, B, T, False, dy=c.dy)
    _compare(f'SIM {name}', (f32.y, f32.dx), f32.grads, (y, dx), {k: sd['g_' + k] for k in R.grad_names(mode)})


def test_case_list_covers_the_edges():
    """The shapes the GPU file is meant to reach are in the list (a guard against a quiet edit of the list)."""
    S = R.CASES
    assert {S[n]['T'] for n in R.names('T')} == {1, 2, 15, 16, 17, 31, 32}
    for n in R.names('T'):
        T = S[n]['T']
        assert {0, min(1, T), T - 1, T} <= set(S[n]['pads'])
    assert {(S[n]['T'], S[n]['d'], S[n]['ldwu']) for n in R.names('d')} == \
        {(T, d, ld) for T in (32, 17) for d in (1, 15, 16, 17, 32) for ld in {R.dpe_of(d), 64}}
    assert all(S[n]['ldg_u'] == S[n]['d'] and S[n]['ldg_d'] == 68 and S[n]['pad_fill'] > 0 for n in R.names('d'))
    assert {(S[n]['mode'], S[n]['inner'], S[n]['act']) for n in R.names('act')} == \
        {(m, i, a) for m, i in ((0, True), (0, False), (1, False)) for a in range(5)}
    assert {(S[n]['B'], S[n]['T']) for n in R.names('big')} == {(600, 32), (600, 17)}
    assert len(R.names('drop')) == 12


def test_exact_mask_differs_from_additive_mask_in_fp64():
    """Why the reference is not `sim_lib._sasrec_block_fn` in fp64: there the additive mask keeps the score, and a fully padded query row no
    longer attends uniformly.  The fp32 evaluations of both forms agree; the fp64 ones do not."""
    c = R.reference('T17')
    d64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in c.desc.items()}
    y_add = sim_lib._sasrec_block_fn(d64, c.x.double(), c.mask, c.T)
    assert float((y_add - c.ref.y).abs().max()) > 1e-2
    y32 = sim_lib._sasrec_block_fn(c.desc, c.x, c.mask, c.T)
    assert float((y32.double() - c.ref.y).abs().max()) < Y_TOL
