"""GPU: every route of a4r_gemm_nt's bf16 and fp32 kernels (csrc/a4r_gemm.hip, a4r_gemm256.hip, a4r_gemm_skinny.hip) and every epilogue form of
dispatch_same against the fp64 reference of tests/gemm_ref.py: small-integer operands bit for bit, random operands within the fp32 summation bound,
every tensor a view with its own leading dimension into a poisoned buffer, the bytes around C and C2 untouched.  Each case first asserts the
precondition that puts it on its route (the route table and the bounds: tests/gemm_ref.py; its soundness: tests/test_gemm_ref_cpu.py)."""
from types import SimpleNamespace

import pytest
import torch

import gemm_ref as G

pytestmark = pytest.mark.gpu

DEFAULT_VARIANT, DEFAULT_TAIL = 2, 3


def dev():
    return torch.device('cuda:0')


@pytest.fixture
def knobs():
    """set(variant, tail_max) for the test; gemm_variant and gemm_tail_max are process-global and go back to what they were"""
    from adapter4rec_amd import _lib as L
    old_v, old_t = L.gemm_variant(-1), L.gemm_tail_max(-1)

    def set_(variant, tail=None):
        L.gemm_variant(variant)
        L.gemm_tail_max(DEFAULT_TAIL if tail is None else tail)
    try:
        yield set_
    finally:
        L.gemm_variant(old_v)
        L.gemm_tail_max(old_t)


def assert_on_route(L, rname, shape, ti, to):
    """the precondition that puts (shape, types) on the route, from the library where it decides, from a4r_gemm_nt's shape rule otherwise"""
    r = G.ROUTES[rname]
    M, N, K = shape
    isz = 4 if ti == 'f32' else 2
    assert L.gemm_variant(-1) == r.variant and L.gemm_tail_max(-1) == (DEFAULT_TAIL if r.tail is None else r.tail)
    exp256, plan = next((e, p) for s, e, p in r.shapes if s == shape)
    # `if (g_variant >= 2 && g.M % 256 == 0 && g.N % 256 == 0 && (g.K * isz) % 128 == 0)` -> a4r_gemm_rows_256 rows on the 256-tile kernel
    takes_256 = r.variant >= 2 and M % 256 == 0 and N % 256 == 0 and (K * isz) % 128 == 0
    if exp256 is not None:
        assert takes_256 and L.gemm_rows_256(M, N) == exp256, (rname, shape, L.gemm_rows_256(M, N))
        assert L.gemm_tail_plan(M, N) == plan, (rname, shape, L.gemm_tail_plan(M, N))
    if rname.startswith('t128'):
        assert r.variant < 2 and L.gemm_rows_256(M, N) == 0   # g_variant 0 / 1: neither the 256-tile nor the skinny kernels are tried
    elif rname == 'skinny_n64':
        # `if (g.N == 64 && g_variant >= 2)`; a4r_gemm_nt_skinny64: `g.N != 64 || g.M % 64 || (g.K * 2) % 128 || g.in_dtype != A4R_BF16` -> 1
        # (`g.dact == A4R_DACT_MULQ8_` -> 1 as well: that form must fall back to the 128-tile kernel and still be right)
        assert N == 64 and r.variant >= 2 and M % 64 == 0 and (K * 2) % 128 == 0 and ti == 'bf16' and not takes_256
    elif rname == 'skinny_k64':
        # `if (g_variant == 2 && g.K == 64 && g.N >= 256)`; a4r_gemm_nt_skinnyk: `g.K != 64 || g.N % 128 || g.M % 64 || in / out != bf16` -> 1,
        # `g.dact != A4R_ACT_NONE` -> 1: then the 128-tile kernel, as long as the 256-tile one does not take the shape
        assert r.variant == 2 and K == 64 and N >= 256 and N % 128 == 0 and M % 64 == 0 and (ti, to) == ('bf16', 'bf16')
        assert not takes_256 or L.gemm_rows_256(M, N) == 0
    elif rname == 'auto_small':
        assert takes_256 and L.gemm_rows_256(M, N) == 0      # `if (head_rows == 0) goto small_tiles;`
    elif rname == 'split':
        assert 0 < L.gemm_rows_256(M, N) < M                 # `if (head_rows < g.M) { split_rows(...) ...`


def device_buffers(c):
    return {k: v.to(dev()) for k, v in c.buf.items()}


def call(L, c, d, M=None, **over):
    f = c.form
    t = lambda nm, on: G.view(c, nm, buf=d) if on else None
    kw = dict(bias=G.bias_of(c, d), C2=t('C2', f.c2 is not None), R1=t('R1', f.r1), R2=t('R2', f.r2), Pre=t('Pre', f.dact), act=f.act, dact=f.dact,
              alpha=f.alpha, drop_p=c.p, drop_site=c.site, drop_seed=c.seed, drop_first=f.drop == 1,
              c2_deriv={None: False, 0: False, 1: True, 'q8': 'q8'}[f.c2], M=M)
    kw.update(over)
    L.gemm_nt(t('A', True), t('B', True), t('C', True), **kw)
    torch.cuda.synchronize()


def complaints(c, d, ref, exp):
    """everything wrong with the buffers d after the call"""
    h = {k: v.cpu() for k, v in d.items()}
    out = G.intact(c, h)
    for k, v in h.items():
        if k not in ('C', 'C2') and not torch.equal(G._bits(v), G._bits(c.buf[k])):
            out.append(f'{c.name}: input {k} changed')
    got = SimpleNamespace(C=G.view(c, 'C', buf=h), C2=G.view(c, 'C2', buf=h) if c.form.c2 is not None else None)
    return out + G.judge(c, got, ref, exp)


CASES = G.route_cases()


@pytest.mark.parametrize('shape,ti,to,kind,form,route', CASES, ids=[f'{r}-{s[0]}x{s[1]}x{s[2]}-{ti}-{to}-{k}-{f}' for s, ti, to, k, f, r in CASES])
def test_gemm_route(shape, ti, to, kind, form, route, knobs):
    from adapter4rec_amd import _lib as L
    r = G.ROUTES[route]
    knobs(r.variant, r.tail)
    assert_on_route(L, route, shape, ti, to)
    c, ref, exp = G.case_and_reference(shape, ti, to, kind, form)
    d = device_buffers(c)
    call(L, c, d)
    bad = complaints(c, d, ref, exp)
    assert not bad, bad


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize('variant,tail', [(0, None), (1, None), (2, None), (4, None), (4, 0)])
def test_gemm_rows_argument_smaller_than_the_tensor(variant, tail, knobs):
    """M = 256 of a 512-row tensor: rows 256.. keep their sentinels (C and C2), the rows in front are right"""
    from adapter4rec_amd import _lib as L
    knobs(variant, tail)
    c, ref, exp = G.case_and_reference((512, 256, 128), 'bf16', 'bf16', 'exact', 'full_relu')
    d = device_buffers(c)
    call(L, c, d, M=256)
    h = {k: v.cpu() for k, v in d.items()}
    for nm, e in (('C', exp.C), ('C2', exp.C2)):
        got = G.view(c, nm, buf=h)
        assert torch.equal(got[:256], e[:256]), nm
        assert bool((got[256:] == G.SENTINEL).all()), f'{nm}: rows behind M written'
    assert G.intact(c, h) == []


@pytest.mark.parametrize('variant,tail,shape', [(0, None, (256, 256, 128)), (1, None, (256, 256, 128)), (2, None, (256, 256, 128)),
                                                (4, None, (256, 256, 128)), (4, 0, (256, 256, 128)), (2, None, (128, 64, 64)),
                                                (2, None, (128, 256, 64))])
def test_gemm_bias_pointer_aligned_to_4_bytes_only(variant, tail, shape, knobs):
    """the 256-tile and skinny kernels load bias in 16-byte pieces only from a 4-byte aligned pointer and otherwise step aside
    (`reinterpret_cast<uintptr_t>(g.bias) & 3u` -> 1); every route must take a bias that is 4- but not 16-byte aligned"""
    from adapter4rec_amd import _lib as L
    knobs(variant, tail)
    for kind in ('exact', 'bounded'):
        c, ref, exp = G.case_and_reference(shape, 'bf16', 'bf16', kind, 'm3')
        d = device_buffers(c)
        moved = torch.full((c.N + 9,), float('nan'), device=dev())
        moved[1:1 + c.N] = G.bias_of(c, d)
        bias = moved[1:1 + c.N]
        assert bias.data_ptr() % 16 == 4
        call(L, c, d, bias=bias)
        bad = complaints(c, d, ref, exp)
        assert not bad, bad


def _rejected(L, c, **over):
    d = device_buffers(c)
    with pytest.raises(RuntimeError):
        call(L, c, d, **over)
    torch.cuda.synchronize()
    for nm in c.pristine:
        assert torch.equal(G._bits(d[nm].cpu()), G._bits(c.pristine[nm])), f'{nm} written by a rejected call'


@pytest.mark.parametrize('variant', [0, 2, 4])
def test_gemm_rejects(variant, knobs):
    """one valid call changed in one respect: an error, and the sentinel-filled outputs as they were"""
    from adapter4rec_amd import _lib as L
    knobs(variant)
    c, ref, exp = G.case_and_reference((256, 256, 128), 'bf16', 'bf16', 'exact', 'full_relu')
    M, N = c.M, c.N
    d = device_buffers(c)
    call(L, c, d)                                            # the valid call
    assert not complaints(c, d, ref, exp)
    flat = torch.zeros(16 + (M + 2) * (N + 8), dtype=torch.bfloat16, device=dev())
    _rejected(L, c, R1=torch.as_strided(flat, (M, N), (N - 8, 1)))                     # ldr1 < N
    _rejected(L, c, C2=torch.as_strided(flat, (M, N), (N + 4, 1)))                     # ldc2 * size % 16 != 0
    _rejected(L, c, dact=G.ACT_RELU)                                                   # Pre missing under a dact
    _rejected(L, c, drop_p=1.0)                                                        # drop_p = 1


def test_gemm_knobs_are_back_at_their_defaults():
    """runs last in this module: what the fixtures restored"""
    from adapter4rec_amd import _lib as L
    assert L.gemm_variant(-1) == DEFAULT_VARIANT and L.gemm_tail_max(-1) == DEFAULT_TAIL
