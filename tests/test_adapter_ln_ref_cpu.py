"""tests/adapter_ln_ref.py proven on the CPU, before the kernels are held to it (tests/test_adapter_ln_kernels_gpu.py):
  * its fp64 chain equals torch autograd of the plainly written module to 1e-12;
  * the bf16 model, and tests/sim_lib.py's fp32 restatement that the engine's host-logic tests run on, pass judge on every case;
  * every mutation of the model that a wrong kernel could amount to FAILS judge on a named case (the output names the bound that caught it);
  * the conditions the yardsticks rest on hold for every case; the case table reaches every kernel instantiation.
"""
import pytest
import torch

import adapter_ln_ref as R
import sim_lib


# ------------------------------------------------------------------ the reference against autograd
def _autograd(c):
    """the module written plainly in fp64; loss = <y, dy> + <the residual stream, dres>"""
    p = {k: t.clone().requires_grad_(True) for k, t in c.W.items() if k in ('bd', 'bu', 'gamma', 'beta')}
    x = c.X64.clone().requires_grad_(True)                                  # the dense output before its dropout
    A = x * c.keepmul if c.keepmul is not None else x
    zp = A @ c.W['Wd'].t() + p['bd']
    zp.retain_grad()
    up = R.act64(zp, c.act) @ c.W['Wu'].t() + c.O64 + (A if c.inner else 0)
    v = up + p['bu']
    v.retain_grad()
    y = torch.nn.functional.layer_norm(v, (c.H,), p['gamma'], p['beta'], c.eps)
    loss = (y * c.dy64).sum()
    if c.dres:                                                              # flags bit 0: is the up-projection's bias part of the stream dres reaches?
        loss = loss + ((v if c.bias_total else up) * c.dres64).sum()
    loss.backward()
    dv = v.grad + (c.dres64 if (c.dres and not c.bias_total) else 0)
    return dict(dv=dv, dzp=zp.grad, dh=x.grad, dgamma=p['gamma'].grad, dbeta=p['beta'].grad, dbias=p['bu'].grad, dbd=p['bd'].grad), y, v


@pytest.mark.parametrize('act', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('inner', [False, True])
@pytest.mark.parametrize('form', ['plain', 'dres_before', 'dres_after', 'from_y', 'dropout'])
def test_reference_matches_autograd(act, inner, form):
    c = R.make_case(f'ag_{act}_{inner}_{form}', H=128, M=32, dirn='bwd', act=act, inner=inner, sums='gbvd', dres=form.startswith('dres'),
                    bias_total=form == 'dres_after', beta_y=form == 'from_y', drop=0.25 if form == 'dropout' else 0.0, seed=7 * act + inner)
    # a consistent chain: zp, v / y and the statistics of THIS forward, unrounded
    c.X64 = c.A64
    if c.keepmul is not None:
        c.A64 = c.X64 * c.keepmul
    f = R.chain_fwd(c, model=False)
    c.zp64, c.v64, c.mean64, c.rstd64 = f.zp, (f.y if c.beta_y else f.v), f.mean, f.rstd
    ref = R.chain_bwd(c, model=False)
    ag, y, v = _autograd(c)
    assert float((f.y - y).abs().max()) < 1e-12 and float((f.v - v).abs().max()) < 1e-12
    for k, t in ag.items():
        e = float((getattr(ref, k) - t).abs().max())
        assert e < 1e-12 * max(1.0, float(t.abs().max())), (k, e)


def test_activation_derivatives():
    x = torch.linspace(-4, 4, 801, dtype=torch.float64)
    x = x[x != 0].clone().requires_grad_(True)
    for a in range(5):
        g, = torch.autograd.grad(R.act64(x, a).sum(), x)
        assert float((g - R.dact64(x.detach(), a)).abs().max()) < 1e-12, a
    for a, f in ((2, torch.nn.functional.gelu), (3, lambda t: torch.nn.functional.gelu(t, approximate='tanh')), (4, lambda t: torch.nn.functional.leaky_relu(t, 0.01))):
        assert float((R.act64(x.detach(), a) - f(x.detach())).abs().max()) < 1e-12, a


# ------------------------------------------------------------------ model and simulated engine under the kernel's bounds
def _line(tag, c, figures):
    return f'{tag} ' + R.table_row(c, figures)


def _as_got(c, m):
    """a chain's output in the form run_fwd / run_bwd deliver"""
    got = {x: getattr(m, x) for x in R.expected(c) if hasattr(m, x)}
    if c.dirn == 'bwd':
        for x in R.SUMS:
            if x in got:
                got[x] = got[x] + 0.5
        return got
    if c.res == 'f32':
        got['y32'] = m.y32.float().double()
    elif c.res in ('lo8', 'lo4'):
        yb = m.y.to(torch.bfloat16)
        of, join = (sim_lib.lo8_of, sim_lib.lo8_join) if c.res == 'lo8' else (sim_lib.lo4_of, sim_lib.lo4_join)
        got['y24' if c.res == 'lo8' else 'y20'] = join(yb, of(m.y32.float(), yb)).double()
    return got


@pytest.mark.parametrize('name', R.names())
def test_bf16_model_passes_judge(name):
    c = R.case(name)
    got = _as_got(c, c.fig.model)
    assert set(got) == set(R.expected(c)), (set(got), R.expected(c))
    figures, fails = R.judge(c, got, c.ref, c.fig)
    print(_line('MODEL', c, figures))
    assert not fails, (name, fails)


@pytest.mark.parametrize('name', [n for n in R.names() if R.CASES[n].get('drop', 0.0) == 0.0])
def test_sim_lib_passes_judge(name):
    """the fp32 restatement the engine's host-logic tests run on, through the same buffers, sentinels and bounds as the kernel"""
    c = R.case(name)
    figures, fails = R.judge(c, R.run(c, sim_lib), c.ref, c.fig)
    print(_line('SIM', c, figures))
    assert not fails, (name, fails)


# ------------------------------------------------------------------ mutation checks
MUTATIONS = [
    # forward
    ('no_bd', 'bd dropped', 'fwd_m48_H768_bf16_identity_vy8'),
    ('no_bu', 'bu dropped', 'fwd_m48_H768_bf16_identity_vy8'),
    ('no_bd', 'bd dropped', 'fwd_m48_H512_bf16_houlsby_gelu_v8'),
    ('no_bu', 'bu dropped', 'fwd_m48_H512_bf16_houlsby_gelu_v8'),
    ('no_res2', 'the second residual dropped', 'fwd_m48_H128_bf16_houlsby_vy'),
    ('ln_rounded', 'the LayerNorm run on the bf16-rounded v', 'fwd_m48_H128_bf16_houlsby_vy'),
    ('ln_rounded', 'the LayerNorm run on the bf16-rounded v', 'fwd_mG1_H1024_f32_pfeiffer_y'),
    ('stale', 'the last tile of a workgroup computed from its previous tile\'s rows', 'fwd_mG1_H768_bf16_identity_vy8'),
    ('stale', 'the last tile of a workgroup computed from its previous tile\'s rows', 'fwd_mG1_H256_lo4_houlsby_vy'),
    # backward
    ('swap8', 'one 8-column piece exchanged between two waves', 'bwd_m48_H768_vit'),
    ('bias_swap', 'dbias taken after dres where before is asked', 'bwd_m48_H256_res_bias'),
    ('bias_swap', 'dbias taken before dres where after is asked', 'bwd_m48_H768_vit'),
    ('act_other', 'act\' of a different act', 'bwd_m48_H768_plain'),        # (relu -> gelu; gelu <-> its tanh form differ by less than a bf16 rounding)
    ('act_other', 'act\' of a different act', 'bwd_m48_H128_g_only'),
    ('inner_flip', 'inner_res ignored', 'bwd_m48_H768_vit'),
    ('inner_flip', 'inner_res added where it is off', 'bwd_m48_H128_ln'),
    ('drop_shift', 'the dropout index shifted by four columns', 'bwd_m48_H512_res_bias'),
    ('no_dres', 'dres not added', 'bwd_m48_H768_vit'),
    ('c1_cw', 'c1 divided by CW instead of H', 'bwd_m48_H768_plain'),
    ('c2_cw', 'c2 divided by CW instead of H', 'bwd_m48_H768_plain'),
    ('c2_cw', 'c2 divided by CW instead of H', 'bwd_mG1_H128_vit'),
    ('no_beta', 'xhat from y without subtracting beta', 'bwd_m48_H768_from_y'),
    ('no_beta', 'xhat from y without subtracting beta', 'bwd_m48_H128_from_y_bias'),
]


@pytest.mark.parametrize('mut,what,name', MUTATIONS, ids=[f'{m}-{n}' for m, _, n in MUTATIONS])
def test_mutation_is_caught(mut, what, name):
    c = R.case(name)
    m = R.bf16_model(c, mut=(mut,))
    figures, fails = R.judge(c, _as_got(c, m), c.ref, c.fig)
    print(f'MUTATION {mut} ({what}) on {name}: caught by ' + ('; '.join(fails) if fails else 'NOTHING'))
    assert fails, f'{what}: judge let it pass on {name}'


def test_mutations_cover_the_list():
    assert {m for m, _, _ in MUTATIONS} == {'no_bd', 'no_bu', 'no_res2', 'ln_rounded', 'stale', 'swap8', 'bias_swap', 'act_other', 'inner_flip', 'drop_shift',
                                          'no_dres', 'c1_cw', 'c2_cw', 'no_beta'}
    both = {R.CASES[n]['bias_total'] for m, _, n in MUTATIONS if m == 'bias_swap'}
    assert both == {False, True}


# ------------------------------------------------------------------ what the yardsticks rest on
def test_rows_are_well_conditioned():
    for n in R.names():
        c = R.case(n)
        if c.offset:
            continue
        assert c.var_ratio >= 1e-3, (n, c.var_ratio)
        if c.beta_y:
            assert float(c.gamma.abs().min()) >= 0.25, n


def test_offset_case_yardstick():
    c = R.case('fwd_offset_H768')
    assert c.var_ratio < 1e-2                                              # it IS the ill-conditioned one: mean^2 ~ 900 x the variance
    rel = c.fig.f32['rstd'] / float(c.fig.model.rstd.min())
    print(f'offset rows: fp32 yardstick mean {c.fig.f32["mean"]:.2e} rstd {c.fig.f32["rstd"]:.2e} ({rel:.2e} relative) y {c.fig.f32["y32"]:.2e}')
    assert rel < 1e-4


def test_column_sum_constant():
    """C_SUM = 4 x the worst ratio of the fp32, one-row-after-the-other, shuffled evaluation of the same sums (recorded in adapter_ln_ref's header)"""
    worst = {}
    for n in R.names('bwd_'):
        c = R.case(n)
        for k, v in R.colsum_ratio(c, c.ref, seed=c.seed).items():
            if v > worst.get(k, (0, ''))[0]:
                worst[k] = (v, n)
    print('COLSUM worst fp32 ratio: ' + ' '.join(f'{k}={v:.3f} ({n})' for k, (v, n) in worst.items()))
    w = max(v for v, _ in worst.values())
    assert 4 * w <= R.C_SUM, (w, R.C_SUM)
    assert R.C_SUM <= 4 * w * 1.25, 'C_SUM is looser than four times the observed ratio'


# ------------------------------------------------------------------ the case table reaches everything
def test_forward_table_coverage():
    rows = R.fwd_sweep()
    assert {(H, res) for H, res, *_ in rows} == {(H, res) for H in R.WIDTHS_FWD for res in R.FWD_RES}
    for mode in R.MODES:
        assert len({H for H, _, m, *_ in rows if m == mode}) >= 2, mode
    outs = {o for *_, o, _ in rows}
    assert {'vy', 'y'} <= outs and any('y' not in o.replace('y8', '') and '8' in o for o in ('v8',) if o in outs)
    assert {R.MODES[m][0] for m in R.MODES} == {0, 1, 2, 3, 4}


def test_backward_table_reaches_every_instantiation():
    """launch_bwd_d: WGB x WDB x DRES without beta_y, (WGB, WDB) = (0, 0) and (0, 1) with it; each at every width and both row counts"""
    want = {(g, v, d, False) for g in (False, True) for v in (False, True) for d in (False, True)} | {(False, False, False, True), (False, True, False, True)}
    assert set(R.INSTANTIATION.values()) == want
    have = {n for n in R.names('bwd_')}
    for tag in ('m48', 'mG1'):
        for H in R.WIDTHS_BWD:
            for form in R.BWD_FORMS:
                assert f'bwd_{tag}_H{H}_{form}' in have
    forms = R.BWD_FORMS
    assert {s for _, s, *_ in forms.values()} >= {'', 'gb', 'b'} and any(s == 'gd' for _, s, *_ in forms.values())
    assert any(d and bt and 'v' in s for d, s, bt, *_ in forms.values()) and any(d and not bt and 'v' in s for d, s, bt, *_ in forms.values())


def test_buffers_are_as_described():
    for n in ('fwd_m48_H128_bf16_houlsby_vy', 'bwd_m48_H768_vit', 'fwd_shared_H512', 'fwd_tight_H256'):
        c = R.case(n)
        for k, b in c.bufs.items():
            vw = R.view(c, k)
            assert vw.data_ptr() % 16 == 0 and (vw.stride(0) * vw.element_size()) % 16 == 0 or k in ('stats', 'res32'), (n, k)
            assert b.shape[0] == c.M + 16
            junk = R.JUNK8 if b.dtype == torch.int8 else R.JUNK
            assert bool((b[c.M:] == junk).all()), (n, k)
            if c.wide and not c.shared and k not in ('zp', 'stats'):
                assert vw.stride(0) > vw.shape[1] and bool((b[:, vw.shape[1] + c.col0[k]:] == junk).all())
    c = R.case('fwd_shared_H512')
    assert c.bufs['A'] is c.bufs['O'] and c.bufs['A'].shape[1] == 2 * 512 + 16
    assert R.view(R.case('fwd_tight_H256'), 'A').is_contiguous()
