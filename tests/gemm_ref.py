"""fp64 reference of a4r_gemm_nt's whole epilogue (include/a4r.h, csrc/a4r_gemm_epi.h), the route / form / case tables of its bf16 and fp32
kernels and the judge.  TEST INFRASTRUCTURE ONLY.  tests/test_gemm_ref_cpu.py proves this file sound on the CPU (mutants, exactness, the route
arithmetic); tests/test_gemm_routes_gpu.py runs the kernels through it.

    pre = alpha (A B^T) + bias ; C2 = pre (c2 0) | act'(pre) (c2 1) | its 8-bit level (c2 'q8')
    v = act(pre) ; v *= act'(Pre) (dact 1 - 4) | Pre (DACT_MUL) | decoded Pre byte (DACT_MUL_Q8)
    v = v keep ks if drop_first ; v += R1 + R2 ; v = v keep ks if not drop_first ; C = v rounded ONCE to the output type
keep is the host restatement of the dropout hash (ln_rows_ref.host_mask -> oracle/dropout_masks.py, kind 'rows'): element
(row + drop_row0) * N + col of the LOGICAL [M, N] output -- N, not ldc -- lots against thr16(p); ks = keep_scale(p).  The mask is absolute: it is
never compared route against route.

LAYOUT (make_case).  Every tensor is a view into a wider flat buffer whose base is offset by exactly 16 bytes, each with a leading dimension of
its own: lda = K + 8, ldb = K + 16, ldc = N + 24, ldc2 = N + 32, ldr1 = N + 40, ldr2 = N + 48, ldpre = N + 64 (elements; all different, none equal
to N or K, every one a multiple of 16 bytes in every element type).  PAD_ROWS rows follow the last logical row.  Padding of the operands (A, B,
bias, R1, R2, Pre) is NaN (0xA5 in the one-byte derivative tensor): one padding element read as data makes the result NaN, which no bound
accepts.  C and C2 are pre-filled with attn_ref.SENTINEL (0xA5 bytes in the 8-bit C2); after the call every byte outside the logical [M, N] must
be unchanged (intact).  'inplace' forms alias R1 to C (ldr1 = ldc there, the only exception).

DATA KINDS.
  exact    small integers: A in [-3, 3], B in [-2, 2], bias / R1 / R2 / Pre in [-8, 8], alpha in {1, 0.5}, p = 0.5 (keep_scale 2), act in
           {none, ReLU}, dact in {none, ReLU, DACT_MUL}.  |A B^T| <= 6 K <= 4608 for K <= 768 and every later value is a multiple of 1/2 below
           2^18: every intermediate is exact in fp32 whatever the summation order, so the kernel output must equal the fp64 result rounded once
           (RNE) to the output type BIT FOR BIT (torch.equal, no tolerance), C2 included (pre-activation, or the 0 / 1 ReLU derivative).
  bounded  random operands at the scales of tests/test_kernels_gpu.py (A ~ N(0, 1), B ~ 0.1 N(0, 1), the rest N(0, 1)), pre-rounded to their
           element types, p = 0.25.  Per element, nothing left out:
               |got - ref| <= half_ulp_out(ref) + e32 + act_term
           half_ulp_out: half a bf16 ulp of ref (0 for fp32 outputs).
           e32 = (K + 4) 2^-24 mag, mag = |alpha| |A| |B|^T + |bias| pushed through the epilogue with absolute values: x L at an activation (L = 1;
           GELU forms L_GELU = max gelu' = 1.129), x (sum of the absolute terms of the multiplier) at a dact, x ks at a dropout, + |R1| + |R2|.  K
           products in any order and four roundings behind them.  The derivative outputs take L2_GELU = max |gelu''| = 2 phi(0) = 0.7979.
           act_term (GELU forms only: act 2, c2 1 / 'q8' under GELU, dact 2).  The kernels evaluate erf by Abramowitz-Stegun 7.1.26 (erf_as,
           csrc/a4r_common.h; the handbook states 1.5e-7).  erf_as64 restates it in fp64; measured against exact erf on [0, 12] (the cases'
           |pre| / sqrt 2 stays below 9) the formula's error is E_AS = 1.394e-7 (tests/test_gemm_ref_cpu.py::test_erf_formula_error recomputes
           it).  Allowed: EA = 2 E_AS on erf -- the factor 2 covers the fp32 evaluation of the polynomial, v_rcp_f32 and v_exp_f32 --, i.e.
           EA / 2 on the normal cdf and on gelu', |x| EA / 2 on gelu(x), pushed through the rest of the epilogue like mag.
           ReLU derivative (c2 1, act 1): exact, except where |pre| is within its own e32 of 0 (either value).
           8-bit derivative forms, the rule of test_gemm_q8_derivative: the stored level within one of the nearest level of the reference
           derivative, the decoded value within half a step (+ the derivative's own e32 + act_term) of it; the dgrad form (DACT_MUL_Q8) is
           bounded with the decoded value of the given bytes as the multiplier.
No other tolerance constants.

ROUTES (ROUTES, route_cases).  How each kernel is reached, restated from a4r_gemm_nt (csrc/a4r_gemm.hip) for 256 CUs by rows_256 / tail_plan
below; the GPU test asserts the same numbers from the library before it runs a case, so a change of dispatch policy cannot silently un-cover a
route.  The split launch (split_rows) is reached only with gemm_tail_max(0) under variant 2: with the default tail a partial last round of
rem * 4 <= ncu tiles always fits short tiles of kp <= 2, and variant 4 never splits (a4r_gemm_rows_256 returns M there).
"""
import functools
from types import SimpleNamespace

import torch

from attn_ref import SENTINEL
from ln_rows_ref import host_mask

DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
NCU = 256                                    # MI355X
PAD_ROWS = 2
SENTU8 = 0xA5
U24 = 2.0 ** -24
E_AS = 1.394e-7                              # measured error of the 7.1.26 formula (module docstring)
EA = 2.0 * E_AS
L_GELU = 1.129                               # max gelu'(x) (x = sqrt 2: 1.12890)
L2_GELU = 0.7979                             # max |gelu''(x)| = 2 phi(0)
Q8_OFF = float(torch.tensor(0.1289, dtype=torch.float32))
Q8_STEP = float(torch.tensor(0.0049326, dtype=torch.float32))
ACT_RELU, ACT_GELU, ACT_TANH, ACT_LEAKY, DACT_MUL, DACT_MUL_Q8 = 1, 2, 3, 4, 15, 14
DROP_SEED, DROP_SITE = 0x5EED1234ABCD, 7
LD_EXTRA = dict(A=8, B=16, C=24, C2=32, R1=40, R2=48, Pre=64)


# ------------------------------------------------------------------ activations in fp64
def erf_as64(z):
    """Abramowitz-Stegun 7.1.26 as erf_as (csrc/a4r_common.h) states it, in the dtype of z"""
    az = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * az)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return torch.copysign(1.0 - poly * torch.exp(-az * az), z)


def erf_formula_error(zmax=12.0, n=1200001):
    z = torch.linspace(0.0, zmax, n, dtype=torch.float64)
    return float((erf_as64(z) - torch.erf(z)).abs().max())


def _phi(x):
    return torch.exp(-0.5 * x * x) * 0.3989422804014327


def _cdf(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))


def _tanh_u(x):
    return 0.7978845608028654 * (x + 0.044715 * x * x * x)


def act_fwd(x, act):
    if act == ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == ACT_GELU:
        return x * _cdf(x)
    if act == ACT_TANH:
        return 0.5 * x * (1.0 + torch.tanh(_tanh_u(x)))
    if act == ACT_LEAKY:
        return torch.where(x > 0, x, 0.01 * x)
    return x


def act_bwd(x, act):
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_GELU:
        return _cdf(x) + x * _phi(x)
    if act == ACT_TANH:
        t = torch.tanh(_tanh_u(x))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x)
    if act == ACT_LEAKY:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.01))
    return torch.ones_like(x)


def act_bwd_abs_terms(x, act):
    """sum of the absolute values of the elementary terms act'(x) is formed from -- 1/2 + erf / 2 + x phi; 1/2 + t / 2 + x (1 - t t) u' / 2 --: what
    the error of its fp32 evaluation scales with (the terms cancel in the tails, where act' is small and its error is not)"""
    if act == ACT_GELU:
        return 0.5 + 0.5 * torch.erf(x * 0.7071067811865476).abs() + (x * _phi(x)).abs()
    if act == ACT_TANH:
        t = torch.tanh(_tanh_u(x))
        return 0.5 + 0.5 * t.abs() + (0.5 * x * (1.0 + t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x)).abs()
    return act_bwd(x, act).abs()


# ------------------------------------------------------------------ forms
def _form(name, kinds='eb', act=0, dact=0, bias=False, c2=None, r1=False, r2=False, drop=0, alpha=1.0, inplace=False):
    """drop: 0 none, 1 before the residuals (drop_first), 2 behind them.  c2: None | 0 | 1 | 'q8'.  kinds: e(xact), b(ounded)."""
    return SimpleNamespace(name=name, kinds=kinds, act=act, dact=dact, bias=bias, c2=c2, r1=r1 or inplace, r2=r2, drop=drop, alpha=alpha,
                           inplace=inplace, q8=(c2 == 'q8' or dact == DACT_MUL_Q8))


FORMS = {f.name: f for f in [
    # the four plain special forms of dispatch_same<bf16_t> (m = 0, 1, 2, 3), alpha 1 and 0.5
    _form('m0'), _form('m0_a', alpha=0.5),
    _form('m1', drop=2), _form('m1_a', drop=2, alpha=0.5),
    _form('m2', r1=True), _form('m2_a', r1=True, alpha=0.5),
    _form('m3', bias=True, drop=1, r1=True), _form('m3_a', bias=True, drop=1, r1=True, alpha=0.5),
    # GELU + C2 alone (m == 8)
    _form('gelu_c2pre', 'b', act=ACT_GELU, bias=True, c2=0),
    _form('gelu_c2der', 'b', act=ACT_GELU, bias=True, c2=1),
    _form('gelu_c2q8', 'b', act=ACT_GELU, bias=True, c2='q8'),
    # derivative and all-purpose forms
    _form('dmul', dact=DACT_MUL), _form('dmul_a', dact=DACT_MUL, alpha=0.5),
    _form('dmulq8', 'b', dact=DACT_MUL_Q8),
    _form('full_relu', act=ACT_RELU, bias=True, c2=1, r1=True, r2=True, drop=2, alpha=0.5),
    _form('relu_c2pre', act=ACT_RELU, bias=True, c2=0, alpha=0.5),
    _form('dgelu_r1', 'b', dact=ACT_GELU, r1=True),
    _form('drelu', dact=ACT_RELU),
    # forms the 256-tile kernel does not instantiate: they fall back to a 128-tile kernel
    _form('tanh', 'b', act=ACT_TANH, bias=True),
    _form('leaky', 'b', act=ACT_LEAKY, bias=True),
    _form('act_dact', act=ACT_RELU, dact=ACT_RELU, bias=True),
    _form('dtanh', 'b', dact=ACT_TANH),
    # in place: C is R1
    _form('inplace', 'e', bias=True, inplace=True), _form('inplace_drop', 'e', bias=True, inplace=True, drop=1, alpha=0.5),
]}
BIG_FORMS = ('m0', 'm3', 'gelu_c2der', 'full_relu')          # the 65 000-row shapes
MIXED_256_FORMS = ('m0_a', 'relu_c2pre')                     # mixed types on the 256-tile route: the plain form, and one that must fall back


def forms_for(kind, to, names=None):
    out = []
    for f in FORMS.values():
        if names is not None and f.name not in names:
            continue
        if kind[0] not in f.kinds or (f.q8 and to != 'bf16'):
            continue
        out.append(f.name)
    return out


# ------------------------------------------------------------------ routes: the host arithmetic of csrc/a4r_gemm.hip / a4r_gemm256.hip
def tail_plan(M, N, tail_max=3, ncu=NCU):
    """a4r_gemm_tail_plan -> (p_full, kp)"""
    if M <= 0 or N < 256:
        return (M // 256 if M > 0 else 0, 0)
    ntm, ntn = M // 256, N // 256
    nt = ntm * ntn
    if not tail_max or ntn > ncu or nt % ncu == 0:
        return (ntm, 0)
    pf = (nt // ncu) * ncu // ntn
    rows = (ntm - pf) * 256
    kmax = 7 if pf == 0 else min(tail_max, 7)
    for k in range(1, kmax + 1):
        if (rows + 32 * k - 1) // (32 * k) * ntn <= ncu:
            return (pf, k)
    return (ntm, 0)


def rows_256(M, N, variant=2, tail_max=3, ncu=NCU):
    """a4r_gemm_rows_256"""
    if variant < 2 or M <= 0 or N <= 0 or M % 256 or N % 256:
        return 0
    ntm, ntn = M // 256, N // 256
    tiles = ntm * ntn
    rem = tiles % ncu
    if tiles * 4 <= ncu and variant == 2:
        return 0
    if tail_plan(M, N, tail_max, ncu)[1]:
        return M
    if tiles > ncu and rem > 0 and rem * 4 <= ncu and rem % ntn == 0 and variant < 4:
        return (ntm - rem // ntn) * 256
    return M


BIG = (65792, 256, 128)                                       # 257 row panels
# route -> variant, tail_max (None: the default, 3), type pairs, [(M, N, K), expected a4r_gemm_rows_256 or None, expected a4r_gemm_tail_plan or None]
_SAME = (('bf16', 'bf16'), ('f32', 'f32'))
_ALL4 = _SAME + (('bf16', 'f32'), ('f32', 'bf16'))
_T128 = [((128, 64, 64), None, None), ((256, 192, 192), None, None),      # launch_bn: BN = 64 (N % 128 != 0) ...
         ((128, 256, 128), None, None), ((128, 128, 320), None, None)]    # ... and BN = 128; 1, 2, 3 and 5 K stages of the four-deep ring (bf16)
ROUTES = {
    't128_reg': SimpleNamespace(variant=0, tail=None, types=_ALL4, shapes=_T128),
    't128_glds': SimpleNamespace(variant=1, tail=None, types=_ALL4, shapes=_T128),
    'skinny_n64': SimpleNamespace(variant=2, tail=None, types=(('bf16', 'bf16'), ('bf16', 'f32')),
                                  shapes=[((128, 64, 64), None, None), ((384, 64, 320), None, None)]),
    'skinny_k64': SimpleNamespace(variant=2, tail=None, types=(('bf16', 'bf16'),),
                                  shapes=[((128, 256, 64), None, None), ((256, 384, 64), None, None)]),
    't256_full': SimpleNamespace(variant=4, tail=0, types=_SAME,
                                 shapes=[((256, 256, 64), 256, (1, 0)), ((256, 256, 192), 256, (1, 0)), ((512, 512, 128), 512, (2, 0)),
                                         ((256, 512, 256), 256, (1, 0))]),
    't256_full_mixed': SimpleNamespace(variant=4, tail=0, types=(('bf16', 'f32'), ('f32', 'bf16')), forms=MIXED_256_FORMS + ('inplace',),
                                       shapes=[((256, 256, 192), 256, (1, 0)), ((512, 512, 128), 512, (2, 0))]),
    't256_short': SimpleNamespace(variant=4, tail=None, types=_SAME,
                                  shapes=[((256, 256, 128), 256, (0, 1)), ((16640, 256, 128), 16640, (0, 3)), ((8448, 256, 128), 8448, (0, 2))]),
    't256_full_short': SimpleNamespace(variant=4, tail=None, types=_SAME, forms=BIG_FORMS + ('inplace',), shapes=[(BIG, 65792, (256, 1))]),
    't256_two_rounds': SimpleNamespace(variant=4, tail=0, types=_SAME, forms=BIG_FORMS + ('inplace',), shapes=[(BIG, 65792, (257, 0))]),
    'split': SimpleNamespace(variant=2, tail=0, types=_SAME, forms=BIG_FORMS + ('inplace',), shapes=[(BIG, 65536, (257, 0))]),
    'auto_256': SimpleNamespace(variant=2, tail=None, types=_SAME, shapes=[((256 * 65, 256, 128), 256 * 65, (0, 3))]),
    'auto_small': SimpleNamespace(variant=2, tail=None, types=_SAME, shapes=[((256, 256, 128), 0, (0, 1))]),
}


def route_cases():
    """[(shape, ti, to, kind, form, route)], ordered so that the cases that share a reference (everything but the route) are neighbours"""
    out = []
    for rname, r in ROUTES.items():
        for shape, _, _ in r.shapes:
            for ti, to in r.types:
                for kind in ('exact', 'bounded'):
                    for f in forms_for(kind, to, getattr(r, 'forms', None)):
                        out.append((shape, ti, to, kind, f, rname))
    order = {n: i for i, n in enumerate(ROUTES)}
    out.sort(key=lambda c: (c[0], c[1], c[2], c[3], list(FORMS).index(c[4]), order[c[5]]))
    return out


# ------------------------------------------------------------------ cases
def _esize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _wide(x, ld, fill, pad_rows=PAD_ROWS):
    """flat buffer: 16 bytes, then (rows + pad_rows) x ld, x in the leading columns of the leading rows"""
    off = 16 // _esize(x.dtype)
    rows, W = x.shape
    flat = torch.full((off + (rows + pad_rows) * ld,), fill, dtype=x.dtype)
    flat[off:].view(rows + pad_rows, ld)[:rows, :W] = x
    return flat


def view(c, nm, buf=None, rows=None, ld=None, cols=None):
    """the logical tensor nm inside its flat buffer (buf: another copy of the buffers, e.g. the device's)"""
    rows_, W, ld_ = c.geom[nm]
    flat = (buf if buf is not None else c.buf)[c.alias.get(nm, nm)]
    ld = ld or ld_
    off = 16 // flat.element_size()
    nrow = (flat.numel() - off) // ld
    return flat[off:off + nrow * ld].view(nrow, ld)[:rows or rows_, :cols or W]


_KEYS = ('A', 'B', 'bias', 'R1', 'R2', 'Pre', 'Pre8')


@functools.lru_cache(maxsize=8)
def _tensor(shape, ti, to, kind, seed, key):
    """operand `key` of a (shape, types, kind): made when a form first asks for it, then shared and never written to"""
    M, N, K = shape
    g = torch.Generator().manual_seed(seed * 16 + _KEYS.index(key))
    sh = dict(A=(M, K), B=(N, K), bias=(N,)).get(key, (M, N))
    if key == 'Pre8':
        return torch.randint(0, 256, sh, generator=g, dtype=torch.uint8)
    if kind == 'exact':
        hi = dict(A=3, B=2).get(key, 8)
        x = torch.randint(-hi, hi + 1, sh, generator=g).float()
    else:
        x = torch.randn(*sh, generator=g) * (0.1 if key == 'B' else 1.0)
    return x.to(DT[ti] if key in 'AB' else torch.float32 if key == 'bias' else DT[to])


@functools.lru_cache(maxsize=2)
def _products(shape, ti, to, kind, seed):
    """the two fp64 products every form of a (shape, types, kind) shares: A B^T and |A| |B|^T (bounded kind)"""
    A, B = _tensor(shape, ti, to, kind, seed, 'A').double(), _tensor(shape, ti, to, kind, seed, 'B').double()
    return A @ B.t(), (A.abs() @ B.abs().t()) if kind == 'bounded' else None


def make_case(shape, ti, to, kind, form, seed=0):
    M, N, K = shape
    f = FORMS[form] if isinstance(form, str) else form
    shape = tuple(shape)
    d = lambda key: _tensor(shape, ti, to, kind, seed, key)     # (made when first asked for)
    S, Sabs = _products(shape, ti, to, kind, seed)
    tO = DT[to]
    c = SimpleNamespace(name=f'{M}x{N}x{K}-{ti}-{to}-{kind}-{f.name}', M=M, N=N, K=K, ti=ti, to=to, kind=kind, form=f, S=S, Sabs=Sabs,
                        p=0.0 if not f.drop else (0.5 if kind == 'exact' else 0.25), seed=DROP_SEED, site=DROP_SITE, buf={}, geom={}, alias={})
    ld = {k: (K if k in 'AB' else N) + e for k, e in LD_EXTRA.items()}
    nan = float('nan')
    c.buf['A'], c.geom['A'] = _wide(d('A'), ld['A'], nan), (M, K, ld['A'])
    c.buf['B'], c.geom['B'] = _wide(d('B'), ld['B'], nan), (N, K, ld['B'])
    if f.bias:
        c.buf['bias'] = torch.cat([torch.full((4,), nan), d('bias'), torch.full((4,), nan)])
    if f.inplace:
        c.buf['C'] = _wide(d('R1'), ld['C'], SENTINEL)
        c.alias['R1'], c.geom['R1'] = 'C', (M, N, ld['C'])
    else:
        c.buf['C'] = _wide(torch.full((M, N), SENTINEL, dtype=tO), ld['C'], SENTINEL)
        if f.r1:
            c.buf['R1'], c.geom['R1'] = _wide(d('R1'), ld['R1'], nan), (M, N, ld['R1'])
    c.geom['C'] = (M, N, ld['C'])
    if f.r2:
        c.buf['R2'], c.geom['R2'] = _wide(d('R2'), ld['R2'], nan), (M, N, ld['R2'])
    if f.c2 is not None:
        if f.c2 == 'q8':
            c.buf['C2'] = _wide(torch.full((M, N), SENTU8, dtype=torch.uint8), ld['C2'], SENTU8)
        else:
            c.buf['C2'] = _wide(torch.full((M, N), SENTINEL, dtype=tO), ld['C2'], SENTINEL)
        c.geom['C2'] = (M, N, ld['C2'])
    if f.dact:
        if f.dact == DACT_MUL_Q8:
            c.buf['Pre'] = _wide(d('Pre8'), ld['Pre'], SENTU8)
        else:
            c.buf['Pre'] = _wide(d('Pre'), ld['Pre'], nan)
        c.geom['Pre'] = (M, N, ld['Pre'])
    c.pristine = {k: c.buf[k].clone() for k in ('C', 'C2') if k in c.buf}
    return c


def bias_of(c, buf=None):
    return (buf if buf is not None else c.buf)['bias'][4:4 + c.N] if c.form.bias else None


# ------------------------------------------------------------------ the reference
def compute(c, dtype=torch.float64, mut=(), split=None, bounds=False):
    """C and C2 (before the store rounding) in `dtype`; bounds=True (fp64 only): the per-element error bounds of the bounded kind as well.
    mut: a wrong kernel (tests/test_gemm_ref_cpu.py).  split: head rows of a split launch (only the 'row0' mutant reads it)."""
    f, M, N, K = c.form, c.M, c.N, c.K
    r = SimpleNamespace(C2=None, eC=None, eC2=None, C2_free=None)
    if dtype == torch.float64 and not ({'kchunk', 'apad'} & set(mut)):
        S = c.S
    else:
        kk = K + 1 if 'apad' in mut else K
        A, B = view(c, 'A', cols=kk).to(dtype), view(c, 'B', cols=kk).to(dtype)
        S = A @ B.t()
        if 'kchunk' in mut:                                  # one 64-wide K chunk missing in the last 256 x 256 tile
            S = S.clone()
            S[M - 256:, N - 256:] -= A[M - 256:, K - 64:] @ B[N - 256:, K - 64:].t()
    alpha = 1.0 if 'noalpha' in mut else f.alpha
    v = S * alpha
    if f.bias:
        b = bias_of(c).to(dtype)
        v = v + b * (2 if 'bias2' in mut else 1)
    if bounds:
        mag = c.Sabs * abs(f.alpha) + (bias_of(c).double().abs() if f.bias else 0.0)
        aerr = torch.zeros_like(mag)
        e_pre = (K + 4) * U24 * mag
    pre = v
    v = act_fwd(pre, f.act)
    if bounds:
        if f.act in (ACT_GELU, ACT_TANH):
            mag = mag * L_GELU
        if f.act == ACT_GELU:
            aerr = 0.5 * EA * pre.abs()
    if f.c2 is not None:
        if 'c2post' in mut:
            r.C2 = v
        elif f.c2 == 0:
            r.C2 = pre
        else:
            r.C2 = act_bwd(pre, f.act)
        if bounds:
            if f.c2 == 0:
                r.eC2 = e_pre
            elif f.act == ACT_GELU:
                r.eC2 = (K + 4) * U24 * (L2_GELU * (c.Sabs * abs(f.alpha) + (bias_of(c).double().abs() if f.bias else 0.0)) + act_bwd_abs_terms(pre, ACT_GELU)) + 0.5 * EA
            else:                                            # ReLU derivative: exact away from 0
                r.eC2 = torch.zeros_like(pre)
                r.C2_free = pre.abs() <= e_pre
    if f.dact:
        if f.dact == DACT_MUL_Q8:
            mult = view(c, 'Pre').to(dtype) * Q8_STEP - Q8_OFF
            mabs = view(c, 'Pre').to(dtype) * Q8_STEP + Q8_OFF
        elif f.dact == DACT_MUL:
            mult = view(c, 'Pre').to(dtype)
            mabs = mult.abs()
        else:
            P = view(c, 'Pre').to(dtype)
            mult, mabs = act_bwd(P, f.dact), act_bwd_abs_terms(P, f.dact)
        if bounds:
            aerr = aerr * mult.abs() + (v.abs() * (0.5 * EA) if f.dact == ACT_GELU else 0.0)
            mag = mag * mabs
        v = v * mult
    if f.drop:
        W = c.geom['C'][2] if 'maskldc' in mut else N
        keep = _mask(c.seed, c.site, M, W, c.p)[:, :N].to(dtype)
        if 'row0' in mut and split:
            keep = torch.cat([keep[:split], keep[:M - split]])
        first = (f.drop == 1) != ('droporder' in mut)
    res = None
    for nm in ('R1', 'R2'):
        if getattr(f, nm.lower()):
            t = view(c, nm, ld=c.geom['C'][2] if (nm == 'R1' and 'r1ldc' in mut) else None).to(dtype)
            res = t if res is None else res + t
    if f.drop and first:
        v = v * keep
        if bounds:
            mag, aerr = mag * keep, aerr * keep
    if res is not None:
        v = v + res
        if bounds:
            mag = mag + res.abs()
    if f.drop and not first:
        v = v * keep
        if bounds:
            mag, aerr = mag * keep, aerr * keep
    r.C = v
    if bounds:
        r.eC = (K + 4) * U24 * mag + aerr
    return r


@functools.lru_cache(maxsize=2)
def _mask(seed, site, M, W, p):
    return host_mask(seed, site, M, W, p)


def truncate_bf16(x32):
    return (x32.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def store(c, r, mut=()):
    """what a kernel that computed r stores: one rounding to the output type (the 8-bit level for c2 'q8')"""
    tO = DT[c.to]
    rnd = (lambda x: truncate_bf16(x)) if ('trunc' in mut and c.to == 'bf16') else (lambda x: x.to(torch.float32).to(tO))
    out = SimpleNamespace(C=rnd(r.C), C2=None)
    if r.C2 is not None:
        out.C2 = q8_level(r.C2).to(torch.uint8) if c.form.c2 == 'q8' else rnd(r.C2)
    return out


def q8_level(d):
    return torch.clamp(torch.round((d + Q8_OFF) / Q8_STEP), 0, 255)


@functools.lru_cache(maxsize=1)
def case_and_reference(shape, ti, to, kind, form):
    """(case, fp64 reference with bounds, expected stored tensors of the exact kind): computed once, shared by every route, never written to"""
    c = make_case(shape, ti, to, kind, form)
    ref = compute(c, bounds=(kind == 'bounded'))
    exp = store(c, ref) if kind == 'exact' else None
    return c, ref, exp


# ------------------------------------------------------------------ the judge
def half_ulp_bf16(ref):
    m, e = torch.frexp(ref.abs())
    return torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), e - 9))


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _worst(bad, err, what):
    i = int(torch.where(bad.reshape(-1), err.reshape(-1).nan_to_num(nan=float('inf')), torch.zeros(())).argmax())
    return f'{what}: {int(bad.sum())}/{bad.numel()} out of bound, worst at {divmod(i, bad.shape[1])}'


def judge(c, got, ref, exp=None):
    """got: SimpleNamespace(C, C2) of the logical tensors as the kernel stored them (CPU).  Returns the list of complaints (empty: passed)."""
    out = []
    f = c.form
    if c.kind == 'exact':
        exp = exp or store(c, ref)
        for nm in ('C', 'C2'):
            g, e = getattr(got, nm), getattr(exp, nm)
            if e is not None and not torch.equal(g, e):     # (values: NaN equals nothing, -0 equals +0)
                bad = ~(g.double() == e.double())
                out.append(_worst(bad, (g.double() - e.double()).abs(), f'{c.name} {nm} (exact)'))
        return out
    hu = half_ulp_bf16(ref.C) if c.to == 'bf16' else 0.0
    err = (got.C.double() - ref.C).abs()
    bad = ~(err <= hu + ref.eC)                              # (NaN fails)
    if bool(bad.any()):
        out.append(_worst(bad, err / (hu + ref.eC), f'{c.name} C'))
    if ref.C2 is not None:
        if f.c2 == 'q8':
            lvl = got.C2.double()
            bad1 = ~((lvl - q8_level(ref.C2)).abs() <= 1)
            err = (lvl * Q8_STEP - Q8_OFF - ref.C2).abs()
            bad2 = ~(err <= 0.5 * Q8_STEP + ref.eC2)
            if bool(bad1.any()):
                out.append(_worst(bad1, (lvl - q8_level(ref.C2)).abs(), f'{c.name} C2 level'))
            if bool(bad2.any()):
                out.append(_worst(bad2, err, f'{c.name} C2 decoded'))
        else:
            hu2 = half_ulp_bf16(ref.C2) if c.to == 'bf16' else 0.0
            err = (got.C2.double() - ref.C2).abs()
            bad = ~(err <= hu2 + ref.eC2)
            if ref.C2_free is not None:                      # ReLU derivative at a pre-activation within its error of 0: 0 or 1
                g2 = got.C2.double()
                bad = bad & ~(ref.C2_free & ((g2 == 0) | (g2 == 1)))
            if bool(bad.any()):
                out.append(_worst(bad, err, f'{c.name} C2'))
    return out


def intact(c, buf):
    """every byte of the C / C2 buffers outside the logical [M, N] is as it was before the call; buf: the buffers after it (CPU)"""
    out = []
    for nm, before in c.pristine.items():
        after = buf[nm].clone()
        view(c, nm, buf={nm: after})[:] = view(c, nm, buf={nm: before})
        if not torch.equal(_bits(after), _bits(before)):
            out.append(f'{c.name}: bytes outside the logical {nm} changed')
    return out


def old_close_accepts(got, ref, dtype):
    """the verdict of close() in tests/test_kernels_gpu.py (its defaults), restated: the judge the NT family had before this file"""
    got, ref = got.float(), ref.float()
    if not bool(torch.isfinite(got).all()):
        return False
    if dtype == torch.float32:
        atol, rtol = 2e-4, 2e-4
    else:
        atol, rtol = 3e-2 * max(1.0, float(ref.abs().max())), 3e-2
    return not bool(((got - ref).abs() > atol + rtol * ref.abs()).any())
