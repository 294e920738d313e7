"""tests/ln_rows_ref.py proven on the CPU, before the kernels are held to it (tests/test_ln_rows_kernels_gpu.py):
  * its fp64 formulas equal torch.nn.functional.layer_norm and its autograd in fp64, on every family of cases;
  * the model (every output rounded once) and tests/sim_lib.py's fp32 restatement pass judge on every case, through the same strided buffers,
    sentinels and bounds as the kernels -- the offset-row cases included: the inputs chosen keep a correct implementation within its bounds;
  * every mutation that a wrong kernel could amount to FAILS on a named case (the output names the bound that caught it);
  * the column-sum constant holds on these cases by the rule that set it; the case table reaches every dispatch branch of a4r_ln_fwd and
    a4r_ln_bwd in both element types.
"""
import types

import pytest
import torch

import ln_rows_ref as R
import sim_lib


# ------------------------------------------------------------------ the reference against layer_norm and its autograd
FAMILIES = ['w_fwd_lean_f32_H520', 'w_fwd_gen_bf16_H504', 'w_sum_f32_H1016', 'w_sum_bf16_H8', 'w_fp8_bf16_H512', 'f_fwd_f32_add1', 'f_fwd_bf16_add40',
            'f_fwd_f32_drop0.5', 'c_fwd_f32_offset_1e-06', 'w_bwd_lean_bf16_H8', 'w_bwd_gen_f32_H520', 'w_bwd_gen_bf16_H1024', 'f_bwd_f32_sums_g',
            'f_bwd_bf16_sums_bv', 'f_bwd_f32_add37', 'f_bwd_bf16_drop0.1', 'f_bwd_f32_dv2_both', 'f_bwd_bf16_dv2_p0', 'c_bwd_f32_offset_1e-12',
            'r_bwd_pg_f32_H72_2048_dres_dv2', 'r_bwd_gen_bf16_H72_M5']


def _x_of(c):
    if c.kind == 'sum':
        return c.x['h'] + c.x['res']
    return c.x['v'] + (c.x['add'][torch.arange(c.M) % c.add_rows] if c.add_rows else 0)


@pytest.mark.parametrize('name', FAMILIES)
def test_reference_matches_layer_norm_autograd(name):
    c = R.case(name)
    x = _x_of(c).clone().requires_grad_(True)
    gamma, beta = c.x['gamma'].clone().requires_grad_(True), c.x['beta'].clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (c.H,), gamma, beta, c.eps)
    keep = c.keep if c.keep is not None else 1.0
    if c.kind != 'bwd':
        ref = c.ref
        assert float((ref['y'] - y.detach() * keep).abs().max()) < 1e-12 * max(1.0, float(y.detach().abs().max()))
        assert float((ref['mean'] - x.detach().mean(-1)).abs().max()) < 1e-12 * max(1.0, float(x.abs().max()))
        var = x.detach().var(-1, unbiased=False)
        assert float((ref['rstd'] * torch.sqrt(var + c.eps) - 1).abs().max()) < 1e-12
        if c.kind == 'sum':
            assert torch.equal(ref['sum'], x.detach()) and torch.equal(ref['sum32'], x.detach()) and torch.equal(ref['y32'], ref['y'])
        return
    # the backward is given stats rounded to fp32: restate it with the stats of THIS x, unrounded, so that autograd sees the same function
    exact = R.compute(c, torch.float64, fwd_only=True)
    c2 = types.SimpleNamespace(**vars(c))
    c2.x = dict(c.x, stats=torch.stack([exact['mean'], exact['rstd']], 1))
    ref = R.compute(c2, torch.float64)
    (y * keep * c.x['dy']).sum().backward()
    dv = x.grad + (c.x['dres'] if c.dres else 0)
    for k, t in (('dv', dv), ('dgamma', gamma.grad), ('dbeta', beta.grad), ('dbias', x.grad.sum(0))):
        assert float((ref[k] - t).abs().max()) < 1e-11 * max(1.0, float(t.abs().max())), k
    if c.dv2:
        assert float((ref['dv2'] - dv * (c.keep2 if c.keep2 is not None else 1.0)).abs().max()) < 1e-11 * max(1.0, float(dv.abs().max()))
    # and the rounding of the stats moves the reference the test uses by no more than fp32 roundoff of its terms
    tol = 2.0 ** -22 * max(1.0, float(exact['mean'].abs().max())) * float(exact['rstd'].max()) * max(1.0, float(ref['dv'].abs().max()))
    assert float((c.ref['dv'] - ref['dv']).abs().max()) < tol


def test_quantiser_reference():
    c = R.case('w_quant_f32_H520')
    q, s = R.quantise(c.ref['yq'])
    amax = c.x['v'].abs().amax(-1)
    assert float(s[3]) == 1.0 and int(q[3].max()) == 0 and float(amax[3]) == 0                           # the row of zeros
    live = amax > 0
    assert float(((s - amax / 448).abs() / (amax / 448).clamp(min=1e-300))[live].max()) < 2.0 ** -23
    deq = q.view(torch.float8_e4m3fn).float().double() * s[:, None]
    assert bool(((deq - c.x['v']).abs() <= 2.0 ** -4 * c.x['v'].abs() * (1 + 2.0 ** -20) + 2.0 ** -10 * s[:, None]).all())
    assert bool((q[1] == 0x7E).all())                                                                   # the constant row: every byte is 448, the e4m3 maximum


# ------------------------------------------------------------------ model and simulated engine under the kernel's bounds
@pytest.mark.parametrize('name', R.names())
def test_model_passes_judge(name):
    c = R.case(name)
    got = c.fig.model
    assert set(got) == set(R.expected(c)), (set(got), R.expected(c))
    figures, fails = R.judge(c, got, c.ref, c.fig)
    print('MODEL ' + R.table_row(c, figures))
    assert not fails, (name, fails)


@pytest.mark.parametrize('name', R.names())
def test_sim_lib_passes_judge(name):
    """the fp32 restatement the engine's host-logic tests run on, through the same buffers, sentinels and bounds as the kernel"""
    c = R.case(name)
    figures, fails = R.judge(c, R.run(c, sim_lib), c.ref, c.fig)
    print('SIM ' + R.table_row(c, figures))
    assert not fails, (name, fails)


def test_offset_rows_are_ill_conditioned_and_still_bounded():
    """mean^2 >> variance: what the fp32 yardstick allows there is far more than on unit rows, and still a small share of the spread"""
    for name, centre in (('c_fwd_f32_offset_1e-12', 1000.0), ('c_fwd_bf16_offset_1e-12', 64.0)):
        c, plain = R.case(name), R.case('w_fwd_lean_' + name.split('_')[2] + '_H768')
        assert abs(float(c.ref['mean'].mean()) - centre) < 2 and 0.5 < float(c.ref['rstd'].mean()) < 2
        by, bp = R.f32_bound(c, c.ref, c.fig, 'y'), R.f32_bound(plain, plain.ref, plain.fig, 'y')
        print(f'OFFSET {name}: fp32 bound of y {by:.2e} (unit rows {bp:.2e}), of mean {R.f32_bound(c, c.ref, c.fig, "mean"):.2e}')
        assert by < 1e-2 and (c.dt == 'bf16' or by > 10 * bp)


# ------------------------------------------------------------------ mutation checks
def _mutant(c, mut):
    """the case evaluated as an fp32 kernel with the slip would: compute in float32, stored as the tensors store"""
    return R.store(c, R.compute(c, torch.float32, mut=(mut,)), mut=(mut,))


MUTATIONS = [
    ('one_pass', 'one-pass variance', 'c_fwd_f32_offset_1e-12'),
    ('one_pass', 'one-pass variance', 'c_fwd_gen_f32_offset_1e-06'),
    ('one_pass', 'one-pass variance', 'c_sum_bf16_offset_1e-12'),
    ('skip_row', 'one row missing from a column sum', 'r_bwd_gen_bf16_H72_M4101'),
    ('skip_row', 'one row missing from a column sum', 'w_bwd_gen_f32_H520'),
    ('skip_row', 'one row missing from a column sum', 'r_bwd_pg_bf16_H72_2049_plain'),
    ('dres_in_dbias', 'dres counted in dbias', 'w_bwd_gen_bf16_H512'),
    ('dres_in_dbias', 'dres counted in dbias', 'r_bwd_gen_f32_H72_M5'),
    ('add_div', 'add[row // add_rows] in place of row % add_rows', 'f_fwd_bf16_add20'),
    ('add_div', 'add[row // add_rows] in place of row % add_rows', 'f_bwd_f32_add20'),
    ('mask_ld', 'mask index built with ld in place of H', 'f_fwd_bf16_drop0.1'),
    ('mask_ld', 'mask index built with ld in place of H', 'f_bwd_f32_drop0.5'),
    ('c1_no_gamma', 'gamma left out of c1', 'w_bwd_lean_bf16_H520'),
    ('c1_no_gamma', 'gamma left out of c1', 'r_bwd_pg_f32_H72_2048_plain'),
    ('scale0', 'scale = 0 for a zero row in the quantiser', 'w_quant_bf16_H520'),
    ('scale0', 'scale = 0 for a zero row in the quantiser', 'c_fp8_f32_zero_1e-12'),
]


@pytest.mark.parametrize('mut,what,name', MUTATIONS, ids=[f'{m}-{n}' for m, _, n in MUTATIONS])
def test_mutation_is_caught(mut, what, name):
    c = R.case(name)
    clean = R.judge(c, _mutant(c, 'none'), c.ref, c.fig)[1]
    assert not clean, f'the unmutated fp32 evaluation fails on {name}: {clean}'
    figures, fails = R.judge(c, _mutant(c, mut), c.ref, c.fig)
    print(f'MUTATION {mut} ({what}) on {name}: caught by ' + ('; '.join(fails) if fails else 'NOTHING'))
    assert fails, f'{what}: judge let it pass on {name}'


class _Stray:
    """sim_lib with one stray write after the launch: into column H of row 0, or into row M, of the first output"""

    def __init__(self, where, M):
        self.where, self.M = where, M

    def __getattr__(self, name):
        f = getattr(sim_lib, name)

        def call(*a, **kw):
            f(*a, **kw)
            out = {'ln_fwd': lambda: a[4] if a[4] is not None else kw['y8'], 'ln_bwd': lambda: a[4], 'ln_fwd_sum': lambda: a[5], 'quant_rows_fp8': lambda: a[1]}[name]()
            if self.where == 'col':
                torch.as_strided(out, (1, out.shape[1] + 1), out.stride(), out.storage_offset())[0, out.shape[1]] = 1
            else:
                out[self.M] = 1
        return call


@pytest.mark.parametrize('where', ['col', 'row'])
@pytest.mark.parametrize('name', ['w_fwd_lean_bf16_H520', 'w_bwd_gen_f32_H8', 'w_sum_bf16_H1024', 'w_fp8_f32_H504', 'w_quant_bf16_H4096', 'w_fp8_bf16_H8'])
def test_stray_write_is_caught(name, where):
    """a write into column H, a write into row M: the sentinels of run() notice either, in every kind of case and in both layouts"""
    c = R.case(name)
    R.run(c, sim_lib)
    with pytest.raises(AssertionError, match='written at or beyond row M' if where == 'row' else 'written outside its columns'):
        R.run(c, _Stray(where, c.M))


def test_mutations_cover_the_list():
    assert {m for m, _, _ in MUTATIONS} == {'one_pass', 'skip_row', 'dres_in_dbias', 'add_div', 'mask_ld', 'c1_no_gamma', 'scale0'}
    assert {R.CASES[n]['dt'] for m, _, n in MUTATIONS if m == 'skip_row'} == {'bf16', 'f32'}


def test_null_sum_region_and_input_writes_are_caught():
    c = R.case('f_bwd_f32_sums_g')

    class Bad:
        def __getattr__(self, name):
            def call(*a, **kw):
                getattr(sim_lib, name)(*a, **kw)
                a[0][0, 0] += 1                                            # dy, an input
            return call
    with pytest.raises(AssertionError, match='input dy was written'):
        R.run(c, Bad())

    class Bad2:
        def __getattr__(self, name):
            def call(*a, **kw):
                g = kw['dgamma']                                           # dbeta is null: its region follows dgamma's, 8 sentinels on
                getattr(sim_lib, name)(*a, **kw)
                torch.as_strided(g, (g.numel() + 9,), (1,), g.storage_offset())[g.numel() + 8] = 0.5
            return call
    with pytest.raises(AssertionError, match='neighbourhood of the sums'):
        R.run(c, Bad2())


# ------------------------------------------------------------------ what the bounds rest on
def test_column_sum_constant():
    """C_SUM (adapter_ln_ref) by the rule that set it, on the cases of this file: 4 x the worst ratio of the fp32, one-row-after-the-other, shuffled
    evaluation of the same sums stays at or below it"""
    worst = {}
    for n in R.names():
        c = R.case(n)
        if c.kind != 'bwd' or not c.sums:
            continue
        for k, v in R.colsum_ratio(c, c.ref, seed=c.seed).items():
            if v > worst.get(k, (0, ''))[0]:
                worst[k] = (v, n)
    print('COLSUM worst fp32 ratio: ' + ' '.join(f'{k}={v:.3f} ({n})' for k, (v, n) in worst.items()))
    w = max(v for v, _ in worst.values())
    assert 4 * w <= R.C_SUM, (worst, R.C_SUM)


def test_buffers_are_as_described():
    for n in ('w_fwd_lean_bf16_H520', 'w_bwd_gen_f32_H504', 'w_sum_f32_H8', 'w_fp8_bf16_H1016', 'f_bwd_bf16_add40', 'w_quant_f32_H4088'):
        c = R.case(n)
        for k, b in c.bufs.items():
            vw = R.view(c, k)
            assert vw.data_ptr() % 16 == 0 and (vw.stride(0) * vw.element_size()) % 8 == 0, (n, k)
            assert b.shape[0] == vw.shape[0] and bool((b[-R.PAD_ROWS:] == R.JUNK).all()), (n, k)
            if k in ('add', 'stats'):
                assert vw.is_contiguous()
            else:
                assert b.shape[0] == c.M + R.PAD_ROWS and (vw.stride(0) * vw.element_size()) % 16 == 0
                assert vw.stride(0) - c.H in (8, 64) and c.col0[k] == (32 if vw.stride(0) - c.H == 64 else 0)
                gap = torch.ones(b.shape[1], dtype=torch.bool)
                gap[c.col0[k]:c.col0[k] + c.H] = False
                assert bool((b[:, gap] == R.JUNK).all())
        assert float(_x_of(c).mean(-1).abs().mean()) > 0.3                     # rows are not zero-mean
    assert {R.CASES[n]['wide'] for n in R.names('w_')} == {8, 64}


# ------------------------------------------------------------------ the case table reaches every branch
def test_every_dispatch_branch_in_both_types():
    """each case classified by the conditions a4r_ln_fwd / a4r_ln_bwd dispatch on (ln_rows_ref.branch); every branch x element type must appear,
    the pg branch on both sides of its row threshold, the general backward with one-sided sums"""
    have = {}
    for n in R.names():
        s = R.CASES[n]
        c = types.SimpleNamespace(**dict(dict(add_rows=0, drop=0.0, sums='', dv2=False), **s))
        have.setdefault((R.branch(c), s['dt']), []).append(n)
    for b in R.BRANCHES:
        for dt in R.DTYPES:
            assert have.get((b, dt)), f'no case reaches {b} in {dt}'
    for dt in R.DTYPES:
        pg = [R.CASES[n] for n in have[('bwd_pg', dt)]]
        assert {2048, 2049} <= {s['M'] for s in pg} and {s['sums'] for s in pg} >= {'g', 'b', 'gb'}
        assert any(s.get('dv2') and s.get('drop2') for s in pg) and any(s.get('dv2') and not s.get('drop2') for s in pg) and any(s.get('dres') for s in pg)
        below = [R.CASES[n] for n in have[('bwd_general<1,0>', dt)] if R.CASES[n]['M'] == 2047]
        assert below, 'M = 2047 with dgamma / dbeta must take the general kernel'
        assert {R.CASES[n]['sums'] for n in have[('bwd_general<1,1>', dt)]} >= {'gv', 'bv', 'gbv'}
        assert any(R.CASES[n]['M'] == 4101 for n in have[('bwd_general<1,1>', dt)])
    assert {R.CASES[n]['H'] for n in R.names('w_fwd_lean')} == set(R.WIDTHS) and {R.CASES[n]['H'] for n in R.names('w_quant')} == set(R.WIDTHS_QUANT)
    assert {R.CASES[n]['add_rows'] for n in R.names('f_fwd_bf16_add')} == {1, 20, 37, 40}
