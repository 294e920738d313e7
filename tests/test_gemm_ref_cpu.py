"""CPU: tests/gemm_ref.py is sound -- its judge accepts an ideal kernel and an fp32 evaluation, rejects ten wrong kernels in both data kinds
(and records what close() of tests/test_kernels_gpu.py, the NT family's judge until now, says to each), its exact kind is exact, its activation
term is what it measures, and its route table follows from the host arithmetic of a4r_gemm_rows_256 / a4r_gemm_tail_plan on 256 CUs."""
import math

import pytest
import torch

import gemm_ref as G

SMALL = (512, 512, 128)                                       # four 256 x 256 tiles, two K chunks
SPLIT = 256                                                   # head rows of the pretended split launch ('row0')

# mutant -> the form it is applied to
MUTANTS = {
    'kchunk': 'm0',              # one 64-wide K chunk missing in one 256 x 256 tile
    'bias2': 'm3',               # bias added twice
    'noalpha': 'm0_a',           # alpha ignored
    'droporder': 'full_relu',    # drop_first misread: the residuals on the wrong side of the dropout (full_relu: drop_first = 0)
    'r1ldc': 'm2',               # R1 read with ldc in place of ldr1
    'maskldc': 'm1',             # the mask index formed from ldc instead of N
    'row0': 'm1',                # drop_row0 ignored in the second half of a split
    'c2post': 'relu_c2pre',      # C2 given the post-activation
    'trunc': 'dmul',             # bf16 output truncated instead of rounded to nearest even
    'apad': 'm0',                # one padding column of A entering the sum
}
# What close() of tests/test_kernels_gpu.py says to the mutant's output (True: it ACCEPTS the wrong kernel), per (mutant, kind, output type).
# On THESE operands (512 x 512 x 128, unit-scale bias and residuals) close() catches the gross mutants -- its 3e-2 max |ref| is a few tenths here --
# and lets the truncating store through, in both kinds: a rounding-mode error, or any error below 3 % of the largest output, was invisible to it.
OLD_ACCEPTS = {(m, kind, t): False for m in MUTANTS for kind in ('exact', 'bounded') for t in ('bf16', 'f32')}
OLD_ACCEPTS.update({('trunc', 'exact', 'bf16'): True, ('trunc', 'bounded', 'bf16'): True})


def _types(m):
    return ('bf16',) if m == 'trunc' else ('bf16', 'f32')


def _mutant(m, kind, t):
    c = G.make_case(SMALL, t, t, kind, MUTANTS[m])
    ref = G.compute(c, bounds=kind == 'bounded')
    got = G.store(c, G.compute(c, mut={m}, split=SPLIT), mut={m})
    return c, ref, got


@pytest.mark.parametrize('kind', ['exact', 'bounded'])
@pytest.mark.parametrize('m', list(MUTANTS))
def test_judge_rejects_mutant(m, kind):
    for t in _types(m):
        c, ref, got = _mutant(m, kind, t)
        assert G.judge(c, G.store(c, ref), ref) == [], 'the unmutated reference passes its own judge'
        assert G.judge(c, got, ref), f'{m} ({kind}, {t}) must be rejected'


@pytest.mark.parametrize('kind', ['exact', 'bounded'])
@pytest.mark.parametrize('m', list(MUTANTS))
def test_old_judge_verdict_recorded(m, kind):
    for t in _types(m):
        c, ref, got = _mutant(m, kind, t)
        old = G.old_close_accepts(got.C, ref.C, G.DT[t])
        if got.C2 is not None:
            old = old and G.old_close_accepts(got.C2, ref.C2, G.DT[t])
        if OLD_ACCEPTS[(m, kind, t)]:
            assert old, f'close() used to accept {m} ({kind}, {t})'
        else:
            assert not old, f'close() used to reject {m} ({kind}, {t})'


def test_old_judge_had_a_gap():
    """the point of the new judge: close() accepted a store that truncates instead of rounding to nearest even, and every error of its size:
    a bias wrong by 0.1 on some columns passes close() and fails the bound"""
    assert OLD_ACCEPTS[('trunc', 'bounded', 'bf16')] and OLD_ACCEPTS[('trunc', 'exact', 'bf16')]
    for kind in ('exact', 'bounded'):
        c = G.make_case(SMALL, 'bf16', 'bf16', kind, 'm3')
        ref = G.compute(c, bounds=kind == 'bounded')
        wrong = G.compute(c)
        wrong.C = wrong.C.clone()
        wrong.C[:, 8:16] += 0.0625                          # (after the dropout: every row of eight columns)
        got = G.store(c, wrong)
        assert G.old_close_accepts(got.C, ref.C, torch.bfloat16) and G.judge(c, got, ref)


def _unique_cases(kind, max_rows):
    seen = []
    for shape, ti, to, k, f, _ in G.route_cases():
        key = (shape, ti, to, f)
        if k == kind and shape[0] <= max_rows and key not in seen:
            seen.append(key)
    return seen


def test_exact_kind_is_exact():
    """fp32 and fp64 evaluations of the reference agree bit for bit for every exact case of at most 1024 rows; the longer cases have the K,
    the value ranges, the types and the forms of a checked one (exactness does not depend on M or N)."""
    checked = set()
    for shape, ti, to, f in _unique_cases('exact', 1024):
        c = G.make_case(shape, ti, to, 'exact', f)
        r64, r32 = G.compute(c), G.compute(c, torch.float32)
        assert r32.C.dtype == torch.float32 and torch.equal(r32.C.double(), r64.C), c.name
        if r64.C2 is not None:
            assert torch.equal(r32.C2.double(), r64.C2), c.name
        assert float(r64.C.abs().max()) < 2 ** 18
        checked.add((shape[2], ti, to, f))
    for shape, ti, to, f in _unique_cases('exact', 10 ** 9):
        assert shape[2] <= 768 and (shape[2], ti, to, f) in checked, (shape, ti, to, f)


def test_judge_accepts_ideal_and_fp32_evaluations():
    """every bounded form: the fp64 result stored once passes, and so does a plain fp32 evaluation (torch's summation order, exact erf)"""
    for t in ('bf16', 'f32'):
        for shape in ((256, 192, 192), (256, 256, 64)):
            for f in G.forms_for('bounded', t):
                c = G.make_case(shape, t, t, 'bounded', f)
                ref = G.compute(c, bounds=True)
                assert bool(torch.isfinite(ref.eC).all())
                assert G.judge(c, G.store(c, ref), ref) == [], c.name
                assert G.judge(c, G.store(c, G.compute(c, torch.float32)), ref) == [], c.name


def test_bound_is_tight_enough_to_see_one_bf16_ulp():
    """one output element moved by one bf16 ulp, one by 2^-12 relative in fp32: rejected"""
    for t, rel in (('bf16', 2.0 ** -7), ('f32', 2.0 ** -12)):
        c = G.make_case((256, 256, 64), t, t, 'bounded', 'gelu_c2der')
        ref = G.compute(c, bounds=True)
        got = G.store(c, ref)
        i = int(ref.C.abs().reshape(-1).argmax())
        got.C.view(-1)[i] = float(got.C.view(-1)[i]) * (1 + rel)
        assert G.judge(c, got, ref)


def test_erf_formula_error():
    m = G.erf_formula_error()
    assert 0.999 * G.E_AS <= m <= G.E_AS <= 1.5e-7, m
    assert G.EA == 2 * G.E_AS
    # the argument range of the cases: |pre| / sqrt 2 far inside [0, 12]
    c = G.make_case((256, 512, 256), 'bf16', 'bf16', 'bounded', 'gelu_c2der')
    assert float((c.S + G.bias_of(c).double()).abs().max()) / math.sqrt(2) < 9
    # erf_as64 differs from exact erf by what the term allows, in the derivative too
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    cdf = 0.5 * (1 + G.erf_as64(x * 0.7071067811865476))
    assert float((x * cdf - G.act_fwd(x, G.ACT_GELU)).abs().div(x.abs().clamp_min(1e-30)).max()) <= 0.5 * G.E_AS * 1.0001
    assert float((cdf + x * G._phi(x) - G.act_bwd(x, G.ACT_GELU)).abs().max()) <= 0.5 * G.E_AS * 1.0001
    assert float(G.act_bwd(x, G.ACT_GELU).max()) <= G.L_GELU and float(G.act_bwd(x, G.ACT_TANH).max()) <= G.L_GELU
    assert 2 * 0.3989422804014327 <= G.L2_GELU + 1e-4


def test_layout_of_a_case():
    c = G.make_case((256, 192, 192), 'bf16', 'bf16', 'bounded', 'full_relu')
    lds = [c.geom[k][2] for k in ('A', 'B', 'C', 'C2', 'R1', 'R2')] + [G.make_case((256, 192, 192), 'bf16', 'bf16', 'bounded', 'dmul').geom['Pre'][2]]
    assert len(set(lds)) == 7 and all(ld not in (192,) for ld in lds)
    for nm in ('A', 'B', 'R1', 'R2'):
        v = G.view(c, nm)
        assert v.data_ptr() - c.buf[nm].data_ptr() == 16 and bool(torch.isfinite(v.float()).all())
        assert int(torch.isnan(c.buf[nm].float()).sum()) == c.buf[nm].numel() - v.numel()
    assert bool((c.buf['C'] == G.SENTINEL).all()) and bool((c.buf['C2'] == G.SENTINEL).all())
    # intact() sees one byte written outside the logical region, and none inside
    after = {k: v.clone() for k, v in c.buf.items()}
    G.view(c, 'C', buf=after)[:] = 1.0
    assert G.intact(c, after) == []
    after['C'][8 + c.geom['C'][2] - 1] = 1.0                 # last padding column of row 0
    assert G.intact(c, after)
    after = {k: v.clone() for k, v in c.buf.items()}
    after['C2'][-1] = 0.0                                    # behind the last row
    assert G.intact(c, after)


def test_route_table_follows_from_the_host_arithmetic():
    for name, r in G.ROUTES.items():
        tail = 3 if r.tail is None else r.tail
        for (M, N, K), exp256, plan in r.shapes:
            assert M % 128 == 0 and N % 64 == 0 and K % 64 == 0 and K <= 768
            if exp256 is not None:
                assert G.rows_256(M, N, r.variant, tail) == exp256, (name, M, N)
                assert G.tail_plan(M, N, tail) == plan, (name, M, N)
            elif r.variant >= 2:
                assert M % 256 or N % 256 or G.rows_256(M, N, r.variant, tail) == 0 or (name == 'skinny_k64' and K == 64 and N >= 256)
    # launch_bn selects both tile widths among the 128-tile shapes
    assert {128 if s[0][1] % 128 == 0 else 64 for s in G.ROUTES['t128_reg'].shapes} == {64, 128}
    # t256_short: the last panel of the (0, 3) plan has 32 rows; a kp = 2 case is there
    assert 16640 - (math.ceil(16640 / 96) - 1) * 96 == 32
    assert {s[2][1] for s in G.ROUTES['t256_short'].shapes} == {1, 2, 3}
    # auto: more than a quarter of the CUs in tiles / not
    assert (256 * 65 // 256) * 4 > G.NCU and 1 * 4 <= G.NCU
    # split: the last panel alone goes to the 128-tile kernel
    M, N, _ = G.BIG
    assert G.rows_256(M, N, 2, 0) == M - 256 and G.rows_256(M, N, 4, 0) == M and G.rows_256(M, N, 2, 3) == M


def test_split_launch_needs_tail_max_0():
    """with the default gemm_tail_max the launch is never split: a4r_gemm_rows_256 is 0 or M for every shape (256 CUs)"""
    for ntn in range(1, 17):
        for ntm in range(1, 1200):
            M, N = ntm * 256, ntn * 256
            for v in (2, 4):
                assert G.rows_256(M, N, v, 3) in (0, M), (M, N, v)
    assert any(0 < G.rows_256(ntm * 256, 768, 2, 0) < ntm * 256 for ntm in range(1, 400))


def test_case_list_covers_every_route_and_form():
    cases = G.route_cases()
    assert {c[5] for c in cases} == set(G.ROUTES)
    small = {c[4] for c in cases if c[5] == 't256_full' and c[1] == 'bf16'}
    assert small == set(G.FORMS)
    for r in ('t256_full_short', 't256_two_rounds', 'split'):
        assert {c[4] for c in cases if c[5] == r} == set(G.BIG_FORMS) | {'inplace'}
    assert {c[4] for c in cases if c[4].startswith('inplace')} and all(c[3] == 'exact' for c in cases if c[4].startswith('inplace'))
    assert {c[5] for c in cases if c[4] == 'inplace'} == set(G.ROUTES)         # C is R1 on every route
