"""fp64 reference of the fused adapter + LayerNorm kernels (a4r_adapter_ln_fwd / a4r_adapter_ln_bwd: csrc/a4r_adapter_fused.hip, include/a4r.h) and
the cases their tests share.  TEST INFRASTRUCTURE ONLY.  tests/test_adapter_ln_ref_cpu.py proves this file sound on the CPU (autograd, mutation
checks), tests/test_adapter_ln_kernels_gpu.py runs the kernels through it.

    forward : zp = A Wd^T + bd ; z = act(zp) ; v = z Wu^T + bu + O [+ A] ; mean, rstd = 1 / sqrt(var + eps) ; y = (v - mean) rstd gamma + beta
    backward: xhat = (v - mean) rstd  or  (y - beta) / gamma ; g = dy gamma ; c1 = sum g / H ; c2 = sum g xhat / H
              dv = rstd (g - c1 - xhat c2) [+ dres] ; dzp = (dv Wu) act'(zp) ; dh = keep (dzp Wd [+ dv])
              dgamma = sum dy xhat ; dbeta = sum dy ; dbias = sum dv (flags bit 0 clear: before dres is added) ; dbd = sum dzp
O is the residual operand that is not A, as the kernel reads it: bf16, fp32 (res32) or the bf16 tensor joined with its byte / nibble plane.

CASES (make_case).  Every tensor that has a leading dimension is a view into a wider buffer (ld = H + 8, or H + 64 starting 32 columns in; every base
16-byte aligned); gap columns and the rows at or beyond M of the inputs hold JUNK, every output buffer is pre-filled with SENTINEL, M is 16 rows
fewer than the buffers have.  A backward case takes v (or y) and stats from the fp64 forward of the same case, rounded as stored (bf16, fp32).

chain(c, model=False) is the reference; chain(c, model=True) is the BF16 MODEL: the same formulas in fp64 with the kernel's storage roundings -- z
rounded as the up-projection's operand, v = the rounding of the sum while the LayerNorm runs on the unrounded sum, dv rounded before dv Wu, dzp
before dzp Wd, dbd and dbias summed from the values before their rounding, every stored tensor rounded once.

BOUNDS (judge).
  * bf16 tensors (zp, z, v, y / dv, dzp, dh), against the fp64 reference: relative RMS error per 16-row tile at most twice the model's on the same
    tile (a model figure of 0 leaves the store rounding, 2^-9); every element within twice the model's maximum error over the case plus one bf16
    ulp of the reference value.
  * stats and the fp32 y32, against fp64: four times the maximum error over the case of the same two-pass formula evaluated in fp32 on the CPU
    (f32_yardstick, computed per case), floor 2^-22 of the case's magnitude.  The fp64 value meant is the LayerNorm of the sum the kernel forms,
    i.e. with z rounded to bf16 as the operand (the model's chain): with the unrounded z the model itself would miss the bound by two orders of
    magnitude.  One more term, computed per row, never assumed: an element of z that lies within delta of a bf16 rounding tie (delta = 2^-21
    sum |A| |Wd| + 2^-18 |z|: what fp32 accumulation of the H products and the fp32 act() can move it by) may round the other way in fp32 than in
    fp64; the row's sum then moves by one bf16 ulp of that element times the column of Wu, and the allowance is exactly that (flip_allowance; its
    median over the rows of a case is 2e-7 .. 1e-6 on the mean, where the LayerNorm run on the rounded v is off by 5e-5 .. 1e-4).
  * column sums (fp32 atomics, any order): |got - (0.5 + ref)| <= model error + C_SUM 2^-24 (0.5 + sum over rows |term|) per column, the terms
    from the reference.  C_SUM = 4 x the worst ratio of the same sums evaluated in fp32 on the CPU, one row after the other in a shuffled order
    (colsum_ratio).  Worst observed over the CPU file's cases: 3.88 (dgamma of bwd_mG1_H768_res_all: 144 additions onto a running sum of ~17;
    dbias 3.01, dbeta 0.36) -> C_SUM = 16; tests/test_adapter_ln_ref_cpu.py recomputes it.  (The kernels' own worst on an MI355X: 1.84.)  The
    model's error is zero for dgamma, dbeta, dbias (summed before any rounding).  dbd is summed from dv AFTER its rounding to bf16 (its terms are
    the H products dv Wu act' behind every dzp): the model's error per column is what that rounding does, and one more term is computed, not
    assumed, as for the statistics: an fp32 dv within delta of a rounding tie (delta = 2^-21 of the magnitudes dv is put together from) may round
    the other way, which moves all 64 sums by one ulp of that element times a row of Wu times act' (chain_bwd: flip_dbd).  A kernel that rounds
    like the model lands AT the model's error wherever that is large; what is tested, and reported, is the share in use of the remainder
    C_SUM 2^-24 sum |term| + flip_dbd.
  * plane forms: bf16 y joined with its byte / nibble plane against fp64 y at 2^-15 / 2^-11 relative plus the fp32 bound above.
  * y8 / ys (e4m3 + row scale): ys against max |y| / 448 at the fp32 bound (relative); the dequantised value within 2^-4 |y| (3 mantissa bits, half
    an ulp) + 2^-10 ys (half a subnormal step) + the fp32 bound.
  * every sentinel outside rows < M and columns < H intact; the regions of null sum pointers intact; inputs unchanged (run_fwd / run_bwd).
"""
import functools
import math
from types import SimpleNamespace

import torch

import sim_lib
from attn_ref import JUNK, SENTINEL, keep_scale, rb

C_SUM = 16.0
WIDTHS_FWD = (128, 256, 512, 768, 1024)
WIDTHS_BWD = (128, 256, 512, 768)
CW = {128: 32, 256: 32, 512: 64, 768: 96, 1024: 128}
# mode -> (act, A is one of the residuals = the adapter's inner residual, A is passed as R2)
MODES = {'houlsby': (1, True, False), 'houlsby_gelu': (2, True, False), 'compacter': (3, False, False), 'pfeiffer': (1, False, False),
         'parallel': (1, True, True), 'identity': (0, True, False), 'leaky': (4, True, False)}
BF_TENSORS = {'fwd': ('zp', 'z', 'v', 'y'), 'bwd': ('dv', 'dzp', 'dh')}
SUMS = ('dgamma', 'dbeta', 'dbias', 'dbd')
SUM_CODE = dict(g='dgamma', b='dbeta', v='dbias', d='dbd')
JUNK8, SENT8, SENTU8 = 77, -77, 0xA5                    # the same two roles in the int8 planes and the e4m3 tensor


# ------------------------------------------------------------------ activations, fp64
def act64(x, a):
    if a == 1:
        return torch.relu(x)
    if a == 2:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    if a == 3:
        return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    if a == 4:
        return torch.where(x > 0, x, 0.01 * x)
    return x


def dact64(x, a):
    if a == 1:
        return (x > 0).to(x.dtype)
    if a == 2:
        return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    if a == 3:
        t = torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3))
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
    if a == 4:
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.01))
    return torch.ones_like(x)


def ulp_bf16(x):
    """one unit in the last place of the bf16 number nearest to |x| (0 for 0)"""
    a = x.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp(min=1e-300))) - 7), torch.zeros_like(a))


# ------------------------------------------------------------------ cases
def _wide(x, rows, wide, fill):
    """x [M, W] -> (buffer [rows, ld], first column): the buffer holds `fill` everywhere else"""
    W = x.shape[1]
    ld, c0 = {0: (W, 0), 8: (W + 8, 0), 64: (W + 64, 32)}[wide]
    buf = torch.full((rows, ld), fill, dtype=x.dtype)
    buf[:x.shape[0], c0:c0 + W] = x
    return buf, c0


def make_case(name, H, M, dirn, mode='houlsby', act=None, res='bf16', out='vy', dres=False, sums='', bias_total=False, inner=None, drop=0.0,
              beta_y=False, wide=8, shared=False, offset=False, seed=0, eps=1e-12, G=8, device='cpu'):
    """dirn 'fwd' / 'bwd'.  res: the residual that is not A as 'bf16', 'f32' (res32 / y32 fp32), 'lo8', 'lo4' (byte / nibble planes).  out: 'vy' both kept,
    'y' (v = None), 'v8' (y = None, y8 / ys instead), 'vy8' (all).  sums: letters of g (dgamma) b (dbeta) v (dbias) d (dbd).  wide: 0 (ld == H), 8, 64.
    shared: A and the other residual are column slices of one [rows, 2 H + 16] buffer.  offset: res32 = 30 + unit noise.  G: the grid the stale-tile
    mutation of the CPU file assumes."""
    m_act, m_inner, a_is_r2 = MODES[mode]
    act = m_act if act is None else act
    inner = m_inner if inner is None else inner
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = torch.bfloat16
    Mb = M + 16
    c = SimpleNamespace(name=name, H=H, M=M, Mb=Mb, dirn=dirn, mode=mode, act=act, res=res, out=out, dres=dres, sums=sums, bias_total=bias_total,
                        inner=inner, a_is_r2=a_is_r2, drop=drop, beta_y=beta_y, wide=wide, shared=shared, offset=offset, seed=seed, eps=eps, G=G,
                        drop_site=3 + seed % 5, drop_seed=0xad4 * 1000003 + seed, bufs={}, col0={}, device=device)
    A = rn(M, H).to(bf)
    x32 = (rn(M, H) + (30.0 if offset else 0.0)).float()                # the other residual's fp32 value
    O = x32.to(bf)
    c.Wd, c.Wu = (rn(64, H) * 0.05).to(bf), (rn(H, 64) * 0.05).to(bf)
    c.bd, c.bu = rn(64) * 0.1, rn(H) * 0.1
    c.gamma = (1 + 0.15 * rn(H)).clamp(min=0.3)
    c.beta = 0.5 * rn(H)
    plane = None
    if res == 'f32':
        plane, o_val = x32, x32.double()
    elif res == 'lo8':
        plane = sim_lib.lo8_of(x32, O)
        o_val = sim_lib.lo8_join(O, plane).double()
    elif res == 'lo4':
        plane = sim_lib.lo4_of(x32, O)
        o_val = sim_lib.lo4_join(O, plane).double()
    else:
        o_val = O.double()
    c.A64, c.O64 = A.double(), o_val
    c.W = dict(Wd=c.Wd.double(), Wu=c.Wu.double(), bd=c.bd.double(), bu=c.bu.double(), gamma=c.gamma.double(), beta=c.beta.double())

    def put(nm, x, fill=JUNK, w=None):
        c.bufs[nm], c.col0[nm] = _wide(x, Mb, wide if w is None else w, fill)
    if dirn == 'fwd':
        if shared:
            buf = torch.full((Mb, 2 * H + 16), JUNK, dtype=bf)
            buf[:M, :H], buf[:M, H + 8:2 * H + 8] = A, O
            c.bufs['A'], c.col0['A'], c.bufs['O'], c.col0['O'] = buf, 0, buf, H + 8
        else:
            put('A', A)
            put('O', O)
        if plane is not None:
            put('res32', plane, fill=JUNK if res == 'f32' else JUNK8)
    f = chain_fwd(c, model=False)
    if dirn == 'bwd':
        put('dy', rn(M, H).to(bf))
        put('v', (f.y if beta_y else f.v).to(bf))
        if dres:
            put('dres', rn(M, H).to(bf))
        put('zp', rn(M, 64).to(bf), w=0)
        st = torch.stack([f.mean, f.rstd], 1).float()
        put('stats', st, w=0)
        c.dy64, c.v64, c.zp64 = (view(c, x)[:M].double() for x in ('dy', 'v', 'zp'))
        c.dres64 = view(c, 'dres')[:M].double() if dres else None
        c.mean64, c.rstd64 = st[:, 0].double(), st[:, 1].double()
        c.keepmul = None
        if drop > 0:
            from oracle.dropout_masks import DropoutStream
            c.keepmul = (DropoutStream(c.drop_seed).mask('rows', c.drop_site, torch.empty(M, H), drop) > 0).double() * keep_scale(drop)
    c.var_ratio = float((1.0 / f.rstd ** 2 / (f.mean ** 2).clamp(min=1e-300)).min())         # min over rows of var / mean^2 (eps is negligible)
    if device != 'cpu':
        to_device(c, device)
    return c


def to_device(c, device):
    c.device = device
    for k in list(c.bufs):
        c.bufs[k] = c.bufs[k].to(device)
    if c.shared and c.dirn == 'fwd':
        c.bufs['O'] = c.bufs['A']
    for k, t in list(vars(c).items()):
        if torch.is_tensor(t):
            setattr(c, k, t.to(device))
    c.W = {k: t.to(device) for k, t in c.W.items()}


def view(c, nm, buf=None):
    """the [rows, W] view of input nm that the entry point is given"""
    b = c.bufs[nm] if buf is None else buf
    W = {'zp': 64, 'stats': 2}.get(nm, c.H // 2 if (nm == 'res32' and c.res == 'lo4') else c.H)
    return b[:, c.col0[nm]:c.col0[nm] + W]


# ------------------------------------------------------------------ the reference (model=False) and the bf16 model (model=True)
def chain_fwd(c, model, mut=()):
    """mut (mutation checks, model only): 'no_bd', 'no_bu', 'no_res2', 'ln_rounded', 'stale' (tile M / 16 - 1 computed from the rows of tile M / 16 - 1 - G)"""
    r = rb if model else (lambda t: t)
    W = c.W
    A, O = c.A64, c.O64
    if 'stale' in mut:
        nt = c.M // 16
        assert nt > c.G
        A, O = A.clone(), O.clone()
        A[(nt - 1) * 16:] = c.A64[(nt - 1 - c.G) * 16:(nt - c.G) * 16]
        O[(nt - 1) * 16:] = c.O64[(nt - 1 - c.G) * 16:(nt - c.G) * 16]
    zp = A @ W['Wd'].t() + (0 if 'no_bd' in mut else W['bd'])
    z = act64(zp, c.act)
    vs = r(z) @ W['Wu'].t() + (0 if 'no_bu' in mut else W['bu'])
    if c.inner:                                         # two residuals: A and the other one
        vs = vs + A + (0 if 'no_res2' in mut else O)
    else:
        vs = vs + O
    src = rb(vs) if 'ln_rounded' in mut else vs
    mean = src.mean(-1)
    rstd = 1.0 / torch.sqrt(((src - mean[:, None]) ** 2).mean(-1) + c.eps)
    y32 = (src - mean[:, None]) * rstd[:, None] * W['gamma'] + W['beta']
    return SimpleNamespace(zp=r(zp), z=r(z), z_exact=z, zp_exact=zp, vs=vs, v=r(vs), y=r(y32), y32=y32, mean=mean, rstd=rstd)


def chain_bwd(c, model, mut=()):
    """mut: 'swap8', 'bias_swap', 'act_other', 'inner_flip', 'drop_shift', 'no_dres', 'c1_cw', 'c2_cw', 'no_beta'"""
    r = rb if model else (lambda t: t)
    W, H = c.W, c.H
    rstd = c.rstd64[:, None]
    if c.beta_y:
        xh = (c.v64 - (0 if 'no_beta' in mut else W['beta'])) / W['gamma']
    else:
        xh = (c.v64 - c.mean64[:, None]) * rstd
    g = c.dy64 * W['gamma']
    c1 = g.sum(-1, keepdim=True) / (CW[H] if 'c1_cw' in mut else H)
    c2 = (g * xh).sum(-1, keepdim=True) / (CW[H] if 'c2_cw' in mut else H)
    dvln = rstd * (g - c1 - xh * c2)
    dv = dvln + c.dres64 if (c.dres and 'no_dres' not in mut) else dvln
    tv = dv if (c.bias_total != ('bias_swap' in mut)) else dvln
    dvs = r(dv)
    # dbd is summed from dv AFTER its rounding: where the fp32 dv (8 unit roundoffs of the magnitudes it is put together from) may round the other way
    # than the fp64 one, all 64 sums move by one ulp of that element times a row of Wu times act' -- flip_dbd [64], exactly that, judge allows it
    mag = rstd * (g.abs() + c1.abs() + g.abs().mean(-1, keepdim=True) + (xh * c2).abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)) + (c.dres64.abs() if c.dres else 0)
    fu = fragile_ulps(dv, 2.0 ** -21 * mag)
    da = dact64(c.zp64, c.act % 4 + 1 if 'act_other' in mut else c.act)
    dzp = (dvs @ W['Wu']) * da
    dzps = r(dzp)
    dh = dzps @ W['Wd']
    if c.inner != ('inner_flip' in mut):
        dh = dh + dvs
    if c.keepmul is not None:
        dh = dh * (torch.roll(c.keepmul, 4, 1) if 'drop_shift' in mut else c.keepmul)
    dhs = r(dh)
    if 'swap8' in mut:                                  # the piece at column 8 of wave 0 <-> the same piece of wave 1
        a, b = 8, CW[H] + 8
        dvs, dhs = dvs.clone(), dhs.clone()
        for t in (dvs, dhs):
            t[:, a:a + 8], t[:, b:b + 8] = t[:, b:b + 8].clone(), t[:, a:a + 8].clone()
    tg = c.dy64 * xh
    return SimpleNamespace(dv=dvs, dzp=dzps, dh=dhs, dgamma=tg.sum(0), dbeta=c.dy64.sum(0), dbias=tv.sum(0), dbd=dzp.sum(0),
                           abs_dgamma=tg.abs().sum(0), abs_dbeta=c.dy64.abs().sum(0), abs_dbias=tv.abs().sum(0), flip_dbd=((fu @ W['Wu'].abs()) * da.abs()).sum(0),
                           abs_dbd=((dvs.abs() @ W['Wu'].abs()) * da.abs()).sum(0))      # (dbd's terms are the H products behind every dzp: fp32 MFMA sums)


def chain(c, model, mut=()):
    return chain_fwd(c, model, mut) if c.dirn == 'fwd' else chain_bwd(c, model, mut)


def reference(c):
    return chain(c, False)


def bf16_model(c, mut=()):
    m = chain(c, True, mut)
    if c.dirn == 'fwd' and '8' in c.out:
        from test_kernels_gpu import _q8_ref
        q, s = _q8_ref(m.y32.float().cpu())
        m.y8, m.ys = q.view(torch.uint8), s
    return m


# ------------------------------------------------------------------ the fp32 yardsticks
def f32_yardstick(c, model):
    """maximum error over the case of mean, rstd and y from the two-pass formula in fp32 on the sum rounded to fp32 (what the kernel holds)"""
    v = model.vs.float()
    mu = v.mean(-1, keepdim=True)
    rs = torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + torch.tensor(c.eps, dtype=torch.float32, device=v.device))
    y = (v - mu) * rs * c.gamma + c.beta
    e = lambda a, b: float((a.double() - b).abs().max())
    return dict(mean=e(mu[:, 0], model.mean), rstd=e(rs[:, 0], model.rstd), y32=e(y, model.y32))


def fragile_ulps(x, delta):
    """ulp_bf16(x) where x lies within delta of a bf16 rounding tie -- where fp32 arithmetic may round it the other way than fp64 --, else 0"""
    u = ulp_bf16(x)
    frac = torch.where(u > 0, x / u.clamp(min=1e-300), torch.zeros_like(x))
    dist = ((frac - torch.floor(frac)) - 0.5).abs() * u                        # distance to the nearest rounding tie
    return torch.where((u > 0) & (dist < delta), u, torch.zeros_like(u))


def flip_allowance(c, model):
    """two [M]: by how much an element of the row's sum, and its mean, may move because an element of z rounds the other way in fp32 (see the header)"""
    z, zp = model.z_exact, model.zp_exact
    # how far the kernel's fp32 z may sit from the fp64 one: its zp is H products summed in fp32 (8 unit roundoffs of the sum of their magnitudes: the
    # typical error is sqrt(H) / H of the worst case H 2^-24), its act() an fp32 erf / tanh approximation (2^-18 relative)
    delta = 2.0 ** -21 * (c.A64.abs() @ c.W['Wd'].abs().t() + c.W['bd'].abs()) + 2.0 ** -18 * torch.maximum(z.abs(), zp.abs())
    fu = fragile_ulps(z, delta)
    return fu @ c.W['Wu'].abs().amax(0), fu @ c.W['Wu'].mean(0).abs()          # per element of the row's sum; of its mean


def colsum_ratio(c, ref, seed=0):
    """The column sums in fp32 on the CPU -- every term from the fp32 formulas, added one row after the other in a shuffled order onto 0.5 -- : the
    worst |sum - (0.5 + ref)| / (2^-24 (0.5 + sum |term|)) per sum."""
    f = lambda t: t.float()
    rstd = f(c.rstd64)[:, None]
    xh = (f(c.v64) - f(c.W['beta'])) / f(c.W['gamma']) if c.beta_y else (f(c.v64) - f(c.mean64)[:, None]) * rstd
    g = f(c.dy64) * f(c.W['gamma'])
    dvln = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    dv = dvln + f(c.dres64) if c.dres else dvln
    dzp = (dv.to(torch.bfloat16).float() @ f(c.W['Wu'])) * dact64(f(c.zp64), c.act)
    terms = dict(dgamma=f(c.dy64) * xh, dbeta=f(c.dy64), dbias=dv if c.bias_total else dvln)
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(seed)).tolist()
    out = {}
    for nm, t in terms.items():
        acc = torch.full((t.shape[1],), 0.5)
        for i in perm:
            acc += t[i]
        out[nm] = float(((acc.double() - 0.5 - getattr(ref, nm)).abs() / (2.0 ** -24 * (0.5 + getattr(ref, 'abs_' + nm)))).max())
    return out


def model_figures(c, ref):
    m = bf16_model(c)
    fig = SimpleNamespace(model=m)
    if c.dirn == 'fwd':
        fig.f32 = f32_yardstick(c, m)
        fig.flip, fig.flip_mean = flip_allowance(c, m)
    return fig


# ------------------------------------------------------------------ judging
def tile_rms(x, r):
    """relative RMS error per 16-row tile, nan where the reference tile is all zero"""
    e = ((x - r) ** 2).reshape(x.shape[0] // 16, -1).sum(-1)
    n = (r ** 2).reshape(x.shape[0] // 16, -1).sum(-1)
    return torch.where(n > 0, torch.sqrt(e / n.clamp(min=1e-300)), torch.full_like(n, math.nan))


def expected(c):
    """names of what a run of the case must deliver"""
    if c.dirn == 'bwd':
        return BF_TENSORS['bwd'] + tuple(SUM_CODE[k] for k in c.sums)
    names = ['zp', 'z', 'mean', 'rstd'] + (['v'] if 'v' in c.out else []) + (['y'] if 'y' in c.out else []) + (['y8', 'ys'] if '8' in c.out else [])
    return tuple(names + ({'f32': ['y32'], 'lo8': ['y24'], 'lo4': ['y20']}.get(c.res, [])))


def judge(c, got, ref, fig):
    """got: dict name -> fp64 tensor of the M rows (expected(c); y24 / y20: bf16 y joined with its plane; y8 uint8).  Returns (figures, failures):
    figures[x] = (max error, the model's, tile RMS at the tile nearest its bound, the model's on that tile) for bf16 tensors; (max error, fp32 bound,
    worst error / bound) for mean and rstd; (max error, worst error / bound) for y32 / y24 / y20 / y8; (max error, worst error in units of
    2^-24 (0.5 + sum |term|), worst share in use of what the bound adds to the model's error) for the column sums."""
    m = fig.model
    figures, fails = {}, []
    missing = [x for x in expected(c) if x not in got]
    if missing:
        fails.append(f'missing: {missing}')
    for x in BF_TENSORS[c.dirn]:
        if x not in got:
            continue
        g, r, mo = got[x], getattr(ref, x), getattr(m, x)
        if not bool(torch.isfinite(g).all()):
            fails.append(f'{x}: non-finite')
            continue
        err, emax_m = (g - r).abs(), float((mo - r).abs().max())
        over = err - (2 * emax_m + ulp_bf16(r))
        if bool((over > 0).any()):
            i = int(over.argmax())
            fails.append(f'{x}: element {divmod(i, g.shape[1])} off by {float(err.view(-1)[i]):.3e}, beyond 2 x the model\'s maximum {emax_m:.3e} + 1 ulp')
        tk, tm = tile_rms(g, r), tile_rms(mo, r)
        lim = torch.where(tm > 0, 2 * tm, torch.full_like(tm, 2.0 ** -9))
        ratio = torch.nan_to_num(tk / lim, nan=0.0)
        w = int(ratio.argmax())
        if float(ratio[w]) > 1:
            fails.append(f'{x}: relative RMS {float(tk[w]):.3e} of tile {w} beyond {float(lim[w]):.3e} = 2 x the bf16 model')
        figures[x] = (float(err.max()), emax_m, float(tk[w]), float(tm[w]))
    if c.dirn == 'fwd':
        mag = dict(mean=float(m.vs.abs().mean(-1).max()), rstd=float(m.rstd.max()), y32=float(m.y32.abs().max()))
        tight = {k: max(4 * fig.f32[k], 2.0 ** -22 * mag[k]) for k in mag}
        gam = float(c.W['gamma'].abs().max())
        xh_max = ((m.vs - m.mean[:, None]) * m.rstd[:, None]).abs().amax(-1)
        allow = dict(mean=fig.flip_mean, rstd=m.rstd ** 2 * fig.flip, y32=gam * m.rstd * fig.flip * (2 + xh_max))
        for x in ('mean', 'rstd'):
            if x in got:
                err = (got[x] - getattr(m, x)).abs()
                worst = float((err / (tight[x] + allow[x])).max())
                if not bool(torch.isfinite(got[x]).all()) or worst > 1:
                    fails.append(f'{x}: max error {float(err.max()):.3e}, {worst:.3g} x its bound (fp32 {tight[x]:.3e} + the row\'s flip allowance)')
                figures[x] = (float(err.max()), tight[x], worst)
        for x, rel in (('y32', 0.0), ('y24', 2.0 ** -15), ('y20', 2.0 ** -11)):
            if x in got:
                err = (got[x] - m.y32).abs()
                lim = tight['y32'] + allow['y32'][:, None] + rel * m.y32.abs()
                if not bool(torch.isfinite(got[x]).all()) or bool((err > lim).any()):
                    fails.append(f'{x}: max error {float(err.max()):.3e}, {float((err / lim).max()):.3g} x its bound ({rel:.1e} relative + fp32 {tight["y32"]:.1e})')
                figures[x] = (float(err.max()), float((err / lim).max()))
        if 'y8' in got:
            amax = m.y32.abs().amax(-1)
            es = (got['ys'] - amax / 448).abs()
            if bool((es > (tight['y32'] + allow['y32']) / 448 + 2.0 ** -23 * amax / 448).any()):
                fails.append(f'ys: max error {float(es.max()):.3e}')
            deq = got['y8'].to(torch.uint8).view(torch.float8_e4m3fn).float().double() * got['ys'][:, None]
            err = (deq - m.y32).abs()
            lim = 2.0 ** -4 * m.y32.abs() * (1 + 2.0 ** -20) + 2.0 ** -10 * got['ys'][:, None] + tight['y32'] + allow['y32'][:, None]
            if not bool(torch.isfinite(deq).all()) or bool((err > lim).any()):
                fails.append(f'y8: dequantised value {float((err / lim).max()):.3g} x its bound')
            same = float((got['y8'].cpu() == m.y8.cpu()).double().mean()) if hasattr(m, 'y8') else math.nan
            figures['y8'] = (float(err.max()), float((err / lim).max()), same)      # (third: share of bytes equal to _q8_ref of the model's y: a figure, fp32 near-ties differ)
    else:
        for x in SUMS:
            if x not in got:
                continue
            r = getattr(ref, x)
            em = (getattr(m, x) - r).abs()
            fp = 2.0 ** -24 * (0.5 + getattr(ref, 'abs_' + x))
            rest = C_SUM * fp + (m.flip_dbd if x == 'dbd' else 0)
            err = (got[x] - 0.5 - r).abs()
            used = (err - em) / rest                                      # the bound is err <= em + rest: the share of `rest` in use
            if not bool(torch.isfinite(got[x]).all()) or bool((used > 1).any()):
                i = int(used.argmax())
                fails.append(f'{x}: column {i} off by {float(err[i]):.3e}: beyond the model\'s {float(em[i]):.3e} by {float(used[i]):.3g} x what fp32 sums and rounding flips allow')
            figures[x] = (float(err.max()), float((err / fp).max()), max(0.0, float(used.max())))
    return figures, fails


# ------------------------------------------------------------------ running a case through an implementation (adapter4rec_amd._lib on the GPU, sim_lib on the CPU)
def _sent(t, s):
    return bool((t == s).all())


def _outbuf(c, W, dtype, sentinel, wide=None):
    wide = c.wide if wide is None else wide
    ld, c0 = {0: (W, 0), 8: (W + 8, 0), 64: (W + 64, 32)}[wide]
    buf = torch.full((c.Mb, ld), sentinel, dtype=dtype, device=c.device)
    return buf, buf[:, c0:c0 + W], c0


def _intact(c, buf, c0, W, sentinel, nm):
    assert _sent(buf[c.M:], sentinel), f'{c.name}: {nm} written at or beyond row M'
    assert _sent(buf[:, :c0], sentinel) and _sent(buf[:, c0 + W:], sentinel), f'{c.name}: {nm} written outside its columns'


def run_fwd(c, L, frag=None, raw=False):
    """the forward of the case through L.adapter_ln_fwd; returns the dict judge takes (raw: the output tensors as stored, for bit comparisons), after the
    sentinel checks and the check that no input changed"""
    bf, H, M = torch.bfloat16, c.H, c.M
    before = {k: b.clone() for k, b in c.bufs.items()}
    A, O = view(c, 'A'), view(c, 'O')
    R1, R2 = ((O, A) if c.a_is_r2 else (A, O)) if c.inner else (O, None)
    o = {}
    o['zp'], o['z'] = _outbuf(c, 64, bf, SENTINEL, 0), _outbuf(c, 64, bf, SENTINEL, 0)
    o['stats'] = _outbuf(c, 2, torch.float32, SENTINEL, 0)
    if 'v' in c.out:
        o['v'] = _outbuf(c, H, bf, SENTINEL)
    if 'y' in c.out:
        o['y'] = _outbuf(c, H, bf, SENTINEL)
    kw = {}
    if '8' in c.out:
        o['y8'] = _outbuf(c, H, torch.uint8, SENTU8)
        o['ys'] = _outbuf(c, 1, torch.float32, SENTINEL, 0)
        kw.update(y8=o['y8'][1], ys=o['ys'][0].view(-1))
    if c.res == 'f32':
        o['y32'] = _outbuf(c, H, torch.float32, SENTINEL)
    elif c.res in ('lo8', 'lo4'):
        o['y32'] = _outbuf(c, H if c.res == 'lo8' else H // 2, torch.int8, SENT8)
    if c.res != 'bf16':
        kw.update(res32=view(c, 'res32'), y32=o['y32'][1])
    gv = lambda nm: o[nm][1] if nm in o else None
    L.adapter_ln_fwd(A, R1, R2, c.Wd, c.bd, c.Wu, c.bu, c.gamma, c.beta, c.eps, c.act, gv('zp'), gv('z'), gv('v'), gv('y'), gv('stats'), M=M, frag=frag, **kw)
    if c.device != 'cpu':
        torch.cuda.synchronize()
    for nm, (buf, vw, c0) in o.items():
        _intact(c, buf, c0, vw.shape[1], {torch.int8: SENT8, torch.uint8: SENTU8}.get(buf.dtype, SENTINEL), nm)
    for k, b in before.items():
        assert torch.equal(b, c.bufs[k]), f'{c.name}: input {k} was written'
    if raw:
        return {nm: vw[:M].clone() for nm, (buf, vw, c0) in o.items()}
    got = {nm: o[nm][1][:M].double() for nm in ('zp', 'z', 'v', 'y') if nm in o}
    got['mean'], got['rstd'] = o['stats'][1][:M, 0].double(), o['stats'][1][:M, 1].double()
    if '8' in c.out:
        got['y8'], got['ys'] = o['y8'][1][:M].clone(), o['ys'][1][:M, 0].double()
    if c.res == 'f32':
        got['y32'] = o['y32'][1][:M].double()
    elif c.res != 'bf16':
        assert 'y' in o, 'the planes of y go with the bf16 tensor'
        join = sim_lib.lo8_join if c.res == 'lo8' else sim_lib.lo4_join
        got['y24' if c.res == 'lo8' else 'y20'] = join(o['y'][1][:M].cpu(), o['y32'][1][:M].cpu()).double().to(c.device)
    return got


def run_bwd(c, L, frag=None, raw=False):
    """the backward of the case through L.adapter_ln_bwd.  The four sums live in one fp32 arena, 8 sentinels between them: a sum asked for starts from
    0.5, the region of a null pointer holds sentinels and must still hold them afterwards."""
    bf, H, M = torch.bfloat16, c.H, c.M
    before = {k: b.clone() for k, b in c.bufs.items()}
    o = dict(dv=_outbuf(c, H, bf, SENTINEL), dzp=_outbuf(c, 64, bf, SENTINEL, 0), dh=_outbuf(c, H, bf, SENTINEL))
    arena = torch.full((3 * (H + 8) + 64 + 16,), SENTINEL, dtype=torch.float32, device=c.device)
    at = dict(dgamma=(8, H), dbeta=(H + 16, H), dbias=(2 * H + 24, H), dbd=(3 * H + 32, 64))
    asked = {SUM_CODE[k] for k in c.sums}
    sums = {}
    for nm in asked:
        sums[nm] = arena[at[nm][0]:at[nm][0] + at[nm][1]]
        sums[nm].fill_(0.5)
    expect = arena.clone()
    WuT, WdT = c.Wu.t().contiguous(), c.Wd.t().contiguous()
    L.adapter_ln_bwd(view(c, 'dy'), view(c, 'v'), view(c, 'stats'), c.gamma, view(c, 'dres') if c.dres else None, view(c, 'zp'), c.act, WuT, WdT,
                     c.inner, o['dv'][1], o['dzp'][1], o['dh'][1], dgamma=sums.get('dgamma'), dbeta=sums.get('dbeta'), dbias=sums.get('dbias'), M=M,
                     drop_p=c.drop, drop_site=c.drop_site, drop_seed=c.drop_seed, dbd=sums.get('dbd'), bias_total=c.bias_total,
                     beta_y=c.beta if c.beta_y else None, frag=frag)
    if c.device != 'cpu':
        torch.cuda.synchronize()
    for nm, (buf, vw, c0) in o.items():
        _intact(c, buf, c0, vw.shape[1], SENTINEL, nm)
    keep = torch.ones_like(arena, dtype=torch.bool)
    for nm in asked:
        keep[at[nm][0]:at[nm][0] + at[nm][1]] = False
    assert torch.equal(arena[keep], expect[keep]), f'{c.name}: the neighbourhood of the sums (null pointers\' regions, gaps) was written'
    for k, b in before.items():
        assert torch.equal(b, c.bufs[k]), f'{c.name}: input {k} was written'
    if raw:
        return {nm: vw[:M].clone() for nm, (buf, vw, c0) in o.items()}
    got = {nm: o[nm][1][:M].double() for nm in o}
    got.update({nm: t.double() for nm, t in sums.items()})
    return got


def run(c, L, frag=None, raw=False):
    return (run_fwd if c.dirn == 'fwd' else run_bwd)(c, L, frag, raw)


# ------------------------------------------------------------------ the case table
CASES = {}


def _add(name, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw, name=name, seed=500 + 11 * len(CASES))


FWD_MODES = tuple(MODES)                                   # the five of AD_MODES (tests/test_kernels_gpu.py), then act 0 and act 4
FWD_RES = ('bf16', 'f32', 'lo8', 'lo4')
FWD_OUT = ('vy', 'y', 'v8', 'vy8')
# the instantiations of adapter_ln_bwd_kernel<.., WGB, WDB, DRES, FY> that launch_bwd_d can pick, and the forms that reach them (at every width)
BWD_FORMS = {
    # form:        (dres, sums,  bias_total, inner, drop, beta_y, act)       instantiation  WGB WDB DRES FY
    'plain':       (False, '',     False, True,  0.0,  False, 1),          #              0   0   0    0
    'bias':        (False, 'vd',   False, True,  0.25, False, 2),          #              0   1   0    0
    'bias_tot':    (False, 'v',    True,  False, 0.0,  False, 4),          #              0   1   0    0   (no dres: both dbias forms are one)
    'ln':          (False, 'gb',   False, False, 0.0,  False, 3),          #              1   0   0    0
    'all':         (False, 'gbvd', False, False, 0.25, False, 4),          #              1   1   0    0
    'g_only':      (False, 'gd',   False, True,  0.0,  False, 0),          #              1   0   0    0   (dbeta null)
    'b_only':      (False, 'b',    False, True,  0.25, False, 1),          #              1   0   0    0   (dgamma null)
    'res':         (True,  'd',    False, True,  0.0,  False, 2),          #              0   0   1    0
    'res_bias':    (True,  'v',    False, False, 0.25, False, 1),          #              0   1   1    0   dbias BEFORE dres
    'res_biastot': (True,  'vd',   True,  True,  0.0,  False, 1),          #              0   1   1    0   dbias AFTER dres
    'res_ln':      (True,  'gb',   False, True,  0.0,  False, 3),          #              1   0   1    0
    'res_all':     (True,  'gbvd', False, True,  0.0,  False, 2),          #              1   1   1    0   dbias BEFORE dres
    'vit':         (True,  'gbvd', True,  True,  0.0,  False, 2),          #              1   1   1    0   the image tower's form (engine_vit.py)
    'res_b_only':  (True,  'bv',   True,  False, 0.25, False, 4),          #              1   1   1    0   (dgamma null)
    'from_y':      (False, '',     False, True,  0.0,  True,  1),          #              0   0   0    1
    'from_y_bias': (False, 'vd',   False, True,  0.25, True,  2),          #              0   1   0    1
}
INSTANTIATION = {f: (('g' in s or 'b' in s), 'v' in s, dres, by) for f, (dres, s, _, _, _, by, _) in BWD_FORMS.items()}
SWEEP_M = ('48', 'G+1')                                    # rows / 16: 3 tiles; one more tile than workgroups


def bwd_spec(form, H, M, **kw):
    dres, sums, bt, inner, drop, by, act = BWD_FORMS[form]
    return dict(dict(H=H, M=M, dirn='bwd', dres=dres, sums=sums, bias_total=bt, inner=inner, drop=drop, beta_y=by, act=act), **kw)


def fwd_sweep():
    """(H, residual form, mode, outputs, wide): every (H, residual form) pair; every mode at three widths"""
    rows = []
    for hi, H in enumerate(WIDTHS_FWD):
        for ri, res in enumerate(FWD_RES):
            i = hi * 4 + ri
            out = FWD_OUT[(hi + ri) % 4]
            if res in ('lo8', 'lo4') and 'y' not in out:
                out = 'vy8'                               # (the planes of y are offsets from the bf16 y)
            rows.append((H, res, FWD_MODES[i % len(FWD_MODES)], out, (8, 64)[i % 2]))
    return rows


def sweep_specs(G):
    """the form sweep at M = 48 and M = 16 (G + 1), G = the CU count (rounded down to 8) of the machine the kernels run on"""
    specs = []
    for tag, M in (('m48', 48), ('mG1', 16 * (G + 1))):
        for H, res, mode, out, wide in fwd_sweep():
            specs.append(dict(name=f'fwd_{tag}_H{H}_{res}_{mode}_{out}', H=H, M=M, dirn='fwd', mode=mode, res=res, out=out, wide=wide, G=G))
        for fi, form in enumerate(BWD_FORMS):
            for hi, H in enumerate(WIDTHS_BWD):
                specs.append(dict(bwd_spec(form, H, M), name=f'bwd_{tag}_H{H}_{form}', wide=(8, 64)[(fi + hi) % 2], G=G))
    return specs


# the cases of the CPU file (G = 8 there: 16 (G + 1) = 144 rows) by name, with fixed seeds
for _s in sweep_specs(8):
    _add(**_s)
_add('fwd_tight_H256', H=256, M=48, dirn='fwd', mode='houlsby', wide=0)
_add('bwd_tight_H256', **bwd_spec('vit', 256, 48), wide=0)
_add('fwd_shared_H512', H=512, M=80, dirn='fwd', mode='houlsby', shared=True)
_add('fwd_offset_H768', H=768, M=80, dirn='fwd', mode='pfeiffer', res='f32', offset=True)


def seed_of(spec):
    """cases built at run time (the sizes depend on the CU count) take the seed of their name"""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(spec['name'])) % 100003


def names(prefix=''):
    return [n for n in CASES if n.startswith(prefix)]


def build(spec, device='cpu'):
    c = make_case(**dict(spec, seed=spec.get('seed', seed_of(spec))), device=device)
    c.ref = reference(c)
    c.fig = model_figures(c, c.ref)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its fp64 reference on the CPU, computed once per process and shared (read-only) by every test that needs it."""
    return build(CASES[name])


def table_row(c, figures):
    """one line of the tables in the two test files' output: the bf16 tensor nearest its tile bound (max error kernel / model, tile RMS kernel / model),
    then every other figure as worst error / bound (column sums: also in units of 2^-24 (0.5 + sum |term|), bound C_SUM)"""
    bf = [x for x in BF_TENSORS[c.dirn] if x in figures]
    w = max(bf, key=lambda x: figures[x][2] / (2 * figures[x][3]) if figures[x][3] > 0 else 0.0)
    f = figures[w]
    row = f'{c.name:<38}{c.M:>6}  {w:<3} {f[0]:.1e} / {f[1]:.1e}  {f[2]:.2e} / {f[3]:.2e} |'
    for x in figures:
        if x in ('mean', 'rstd'):
            row += f' {x} {figures[x][0]:.1e} ({figures[x][2]:.2f})'
        elif x in ('y32', 'y24', 'y20', 'y8'):
            row += f' {x} {figures[x][0]:.1e} ({figures[x][1]:.2f})'
        elif x in SUMS:
            row += f' {x} {figures[x][1]:.2f} u ({figures[x][2]:.2f})'
    return row


def near_bound(figures, share=0.8):
    """the figures that came within 20 % of their bound"""
    out = []
    for x, f in figures.items():
        r = (f[2] / (2 * f[3]) if f[3] > 0 else 0.0) if len(f) == 4 else f[2] if (x in SUMS or x in ('mean', 'rstd')) else f[1]
        if r > share:
            out.append(x)
    return out
