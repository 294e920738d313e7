"""fp64 reference of the stand-alone LayerNorm family and the row helpers around it (a4r_ln_fwd, a4r_ln_bwd, a4r_ln_fwd_sum, a4r_ln_fwd_fp8,
a4r_quant_rows_fp8: csrc/a4r_rows.hip, include/a4r.h) and the cases their tests share.  TEST INFRASTRUCTURE ONLY.  tests/test_ln_rows_ref_cpu.py
proves this file sound on the CPU (autograd, the fp32 restatement, mutation checks, branch coverage); tests/test_ln_rows_kernels_gpu.py runs the
kernels through it.

    forward (kinds 'fwd', 'fp8', 'sum'):
              x = v [+ add[row % add_rows]]  or  h + res ; mean = sum x / H ; rstd = 1 / sqrt(sum (x - mean)^2 / H + eps)
              y = ((x - mean) rstd gamma + beta) keep ks ; y8 / ys from y (below) ; sum / sum32 = x ; y32 = y
    backward ('bwd'):
              x = v [+ add[row % add_rows]] ; xhat = (x - mean) rstd ; d = dy keep ks ; g = d gamma ; c1 = sum g / H ; c2 = sum g xhat / H
              dv = rstd (g - c1 - xhat c2) [+ dres] ; dgamma = sum_rows d xhat ; dbeta = sum_rows d ; dbias = sum_rows dv BEFORE dres
              dv2 = dv keep2 ks2
    fp8 rows ('quant', and y8 / ys of 'fp8'):
              ys = max |y| / 448, or 1 for a row of zeros ; y8 = e4m3(y / ys), or 0 for a row of zeros
keep is the host restatement of the dropout hash (oracle/dropout_masks.py, kind 'rows': element row * H + col of the LOGICAL [M, H] tensor, lots
against thr16(p)), ks its keep_scale(p), the fp32 number the kernels multiply by.  A backward case takes mean and rstd from the fp64 forward of its
own x, rounded to fp32 as the forward kernels store them.

CASES (make_case).  Every tensor that has a leading dimension is a view into a wider buffer: ld = H + 8, or ld = H + 64 starting 32 columns in
(the e4m3 tensor: 8 / 64 bytes, on an 8-byte-aligned base); every other base is 16-byte aligned.  Gap columns and the rows at or beyond M of the
inputs hold JUNK, every output buffer is pre-filled with SENTINEL (0xA5 in the e4m3 tensor), the buffers have 5 rows more than M.  The column sums
live in one fp32 arena between sentinels and start at 0.5; the region of a null sum pointer holds sentinels and must keep them.  gamma, beta, add
and stats are contiguous, as the kernels read them (add at leading dimension H, stats as [M, 2]); their buffers too carry junk / sentinel rows
beyond what is read.  Rows are NOT zero-mean (every row has its own offset of unit scale): a one-pass variance is visibly worse.  cond:
'offset' rows of mean 1000 (fp32) / 64 (bf16) and unit spread; 'const' row 1 is the constant 2 (variance 0: rstd = eps^-1/2, y = beta exactly)
and row 3 is all zeros; 'zero' the same rows with beta = 0, so that the quantiser inside a4r_ln_fwd_fp8 meets rows of zeros.

compute(c, dtype) evaluates the formulas above in `dtype`: torch.float64 is the reference, torch.float32 the fp32 yardstick (the same two-pass
formula, torch's own reductions).  store(c, values) rounds every output once as its tensor stores it: that is the BF16 MODEL when applied to the
fp64 values.  dv2 comes out of the same launch as dv: the model rounds it once from the UNROUNDED dv.

BOUNDS (judge) -- the project's rules, as tests/adapter_ln_ref.py states them, not new numbers:
  * fp32 outputs (every output of the fp32 instantiations; mean, rstd, sum32, y32 of the bf16 ones) against fp64: four times the maximum error
    over the case of compute(c, float32), floor 2^-22 of the case's magnitude (the largest |reference| of that tensor).
  * bf16 outputs (y, sum, dv, dv2) against fp64: relative RMS error per 16-row tile (the last one ragged) at most twice the model's on the same
    tile (a model figure of 0 leaves the store rounding, 2^-9); every element within twice the model's maximum error over the case plus one bf16
    ulp of the reference value.
  * column sums (fp32 atomics, any order): |got - (0.5 + ref)| <= C_SUM 2^-24 (0.5 + sum over rows |term|) per column, the terms from the
    reference, C_SUM = adapter_ln_ref.C_SUM = 16.  tests/test_ln_rows_ref_cpu.py recomputes adapter_ln_ref's rule on THESE cases (the sums in
    fp32 on the CPU, one row after the other in a shuffled order onto 0.5, for the sums the case asks for) and asserts 4 x the worst ratio
    <= C_SUM; worst observed there: dgamma 3.66 (f_bwd_f32_dv2_both), dbeta 3.27 (r_bwd_pg_f32_H72_2049_plain: 2049 additions onto one running
    sum), dbias 2.83 (f_bwd_f32_drop0.5) -> 14.6 <= 16: the constant stands.  (The kernels' own worst on an MI355X: 2.58.)
  * e4m3 outputs: the y8 / ys rule of adapter_ln_ref: ys against max |y| / 448 (1 for a row of zeros) at the fp32 bound of y over 448 plus
    2^-23 relative; the dequantised value within 2^-4 |y| (3 mantissa bits, half an ulp) + 2^-10 ys (half a subnormal step) + the fp32 bound of
    y.  a4r_quant_rows_fp8 reads y itself: the fp32 bound is 0 there.  A row of zeros: ys == 1 and every byte 0, exactly.
  * masks: the set of zeroed elements equals the host mask exactly (elements whose unmasked reference is 0 aside: there are none but in the
    'const' / 'zero' rows, which carry no dropout).
  * everything: sentinels intact outside rows < M and columns < H, regions of null pointers intact, inputs unchanged (run).

DISPATCH (branch).  The conditions of a4r_ln_fwd / a4r_ln_bwd, restated: forward 'lean' iff no add, thr16(drop_p) == 0 and no y8, else
'general'; backward 'lean' iff no sum, no add, thr16(drop_p) == 0 and no dv2; 'pg' iff dgamma or dbeta, no dbias, no add, thr16(drop_p) == 0
and M >= 2048; else 'general<WGB,WDB>' with WGB = dgamma or dbeta, WDB = dbias.
"""
import functools
import math
from types import SimpleNamespace

import torch

import adapter_ln_ref as A
from attn_ref import JUNK, SENTINEL, rb

C_SUM = A.C_SUM
SENTU8 = A.SENTU8
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
SUM_CODE = dict(g='dgamma', b='dbeta', v='dbias')
SUMS = ('dgamma', 'dbeta', 'dbias')
T_OUT = ('y', 'sum', 'dv', 'dv2')                          # outputs in the case's element type
F32_OUT = ('mean', 'rstd', 'sum32', 'y32')                 # always fp32
PG_MIN_ROWS = 2048
PAD_ROWS = 5


def thr16(p):
    from oracle.dropout_masks import thr16 as t
    return t(p)


def host_mask(seed, site, M, W, p):
    """keep * keep_scale [M, W] fp64 from the host restatement of the hash, element row * W + col"""
    from oracle.dropout_masks import DropoutStream
    return DropoutStream(seed).mask('rows', site, torch.empty(M, W), p).double()


# ------------------------------------------------------------------ cases
def _layout(W, wide):
    return {0: (W, 0), 8: (W + 8, 0), 64: (W + 64, 32)}[wide]


def _wide(x, rows, wide, fill):
    ld, c0 = _layout(x.shape[1], wide)
    buf = torch.full((rows, ld), fill, dtype=x.dtype, device=x.device)
    buf[:x.shape[0], c0:c0 + x.shape[1]] = x
    return buf, c0


def make_case(name, kind, H, M, dt='bf16', wide=8, add_rows=0, drop=0.0, sums='', dres=False, dv2=False, drop2=0.0, res32=False,
              outs=('sum', 'sum32', 'y32'), y=True, cond='', eps=1e-12, seed=0, device='cpu'):
    """kind 'fwd' (a4r_ln_fwd), 'fp8' (a4r_ln_fwd_fp8; y: the T output too), 'sum' (a4r_ln_fwd_sum; res32: the fp32 residual; outs: the optional
    outputs asked for), 'bwd' (a4r_ln_bwd; sums: letters of g b v; dv2 with drop2), 'quant' (a4r_quant_rows_fp8, H up to 4096)."""
    assert kind in ('fwd', 'fp8', 'sum', 'bwd', 'quant') and H % 8 == 0
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    T = DT[dt]
    Mb = M + PAD_ROWS
    c = SimpleNamespace(name=name, kind=kind, H=H, M=M, Mb=Mb, dt=dt, T=T, wide=wide, add_rows=add_rows, drop=drop, sums=sums, dres=dres, dv2=dv2,
                        drop2=drop2, res32=res32, outs=tuple(outs) if kind == 'sum' else (), y=y, cond=cond, eps=eps, seed=seed, device=device,
                        drop_site=3 + seed % 5, drop_seed=0x1f5 * 1000003 + seed, drop2_site=11 + seed % 7, drop2_seed=0x2e3 * 1000003 + seed,
                        bufs={}, col0={}, x={}, keep=None, keep2=None)
    centre, spread = 0.0, 1.0
    if 'offset' in cond:
        centre = 1000.0 if dt == 'f32' else 64.0
    x = (rn(M, H) * spread + rn(M, 1) + centre).to(T)               # rows with their own mean: not zero-mean
    if ('const' in cond or 'zero' in cond) and M >= 4:
        x[1] = 2.0
        x[3] = 0.0
    gamma = (1 + 0.15 * rn(H)).clamp(min=0.3)
    beta = 0.5 * rn(H)
    if 'zero' in cond:
        beta = torch.zeros_like(beta)

    def put(nm, t, w=None, fill=JUNK):
        c.bufs[nm], c.col0[nm] = _wide(t, t.shape[0] + PAD_ROWS, wide if w is None else w, fill)
        c.x[nm] = t.double()
    c.gamma, c.beta = gamma, beta
    c.x['gamma'], c.x['beta'] = gamma.double(), beta.double()
    if kind == 'sum':
        put('h', (x.float() * 0.5).to(T))
        put('res', (x.float() * 0.5 + rn(M, H)).to(torch.float32 if res32 else T))
    elif kind == 'quant':
        put('v', x)
    else:
        put('v', x)
        if add_rows:
            put('add', rn(add_rows, H), w=0)
    if kind == 'bwd':
        put('dy', rn(M, H).to(T))
        if dres:
            put('dres', rn(M, H).to(T))
        f = compute(c, torch.float64, fwd_only=True)
        put('stats', torch.stack([f['mean'], f['rstd']], 1).float(), w=0)
    c.keep = host_mask(c.drop_seed, c.drop_site, M, H, drop).to(device) if drop > 0 else None
    c.keep2 = host_mask(c.drop2_seed, c.drop2_site, M, H, drop2).to(device) if (dv2 and drop2 > 0) else None
    return c


def view(c, nm, buf=None):
    """the [rows, W] view of input nm that the entry point is given"""
    b = c.bufs[nm] if buf is None else buf
    W = 2 if nm == 'stats' else c.H
    return b[:, c.col0[nm]:c.col0[nm] + W]


def branch(c):
    """which kernel the C entry point launches for the case: the conditions of a4r_ln_fwd / a4r_ln_bwd restated (see the header)"""
    thr = thr16(c.drop) > 0
    if c.kind in ('fwd', 'fp8'):
        return 'fwd_general' if (c.add_rows or thr or c.kind == 'fp8') else 'fwd_lean'
    if c.kind == 'bwd':
        wgb, wdb = ('g' in c.sums or 'b' in c.sums), 'v' in c.sums
        if not wgb and not wdb and not c.add_rows and not thr and not c.dv2:
            return 'bwd_lean'
        if wgb and not wdb and not c.add_rows and not thr and c.M >= PG_MIN_ROWS:
            return 'bwd_pg'
        return f'bwd_general<{int(wgb)},{int(wdb)}>'
    return c.kind
BRANCHES = ('fwd_lean', 'fwd_general', 'bwd_lean', 'bwd_pg', 'bwd_general<0,0>', 'bwd_general<0,1>', 'bwd_general<1,0>', 'bwd_general<1,1>')


# ------------------------------------------------------------------ the formulas, in fp64 (reference) or fp32 (yardstick, mutants)
def compute(c, dtype=torch.float64, mut=(), fwd_only=False):
    """name -> [M, ...] tensor in `dtype`, every output unrounded.  mut (tests/test_ln_rows_ref_cpu.py): 'one_pass', 'skip_row', 'dres_in_dbias',
    'add_div', 'mask_ld', 'c1_no_gamma', 'scale0'."""
    X = {k: t.to(dtype) for k, t in c.x.items()}
    H, M = c.H, c.M
    o = {}
    if c.kind == 'quant':
        o['yq'] = X['v']
        return o
    if c.kind == 'sum':
        x = X['h'] + X['res']
    else:
        x = X['v']
        if c.add_rows:
            r = torch.arange(M, device=x.device)
            x = x + X['add'][(r // c.add_rows).clamp(max=c.add_rows - 1) if 'add_div' in mut else r % c.add_rows]
    keep = c.keep
    if keep is not None and 'mask_ld' in mut:
        keep = host_mask(c.drop_seed, c.drop_site, M, _layout(H, c.wide)[0], c.drop)[:, :H].to(x.device)
    if c.kind != 'bwd' or fwd_only:
        mean = x.mean(-1, keepdim=True)
        var = ((x * x).mean(-1, keepdim=True) - mean * mean).clamp(min=0) if 'one_pass' in mut else ((x - mean) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + torch.tensor(c.eps, dtype=dtype, device=x.device))
        o['mean'], o['rstd'] = mean[:, 0], rstd[:, 0]
        if fwd_only:
            return o
        y = (x - mean) * rstd * X['gamma'] + X['beta']
        if keep is not None:
            y = y * keep.to(dtype)
        if c.kind == 'sum':
            o['y'], o['sum'], o['sum32'], o['y32'] = y, x, x, y
        elif c.kind == 'fp8':
            o['y'], o['yq'] = y, y
        else:
            o['y'] = y
        return o
    mean, rstd = X['stats'][:, 0:1], X['stats'][:, 1:2]
    xh = (x - mean) * rstd
    d = X['dy'] * keep.to(dtype) if keep is not None else X['dy']
    gm = d * X['gamma']
    c1 = (d if 'c1_no_gamma' in mut else gm).mean(-1, keepdim=True)
    c2 = (gm * xh).mean(-1, keepdim=True)
    dvln = rstd * (gm - c1 - xh * c2)
    dv = dvln + X['dres'] if c.dres else dvln
    tb = dv if 'dres_in_dbias' in mut else dvln
    terms = dict(dgamma=d * xh, dbeta=d, dbias=tb)
    rows = torch.ones(M, 1, dtype=dtype, device=x.device)
    if 'skip_row' in mut:
        rows[M // 2] = 0
    o['dv'] = dv
    if c.dv2:
        o['dv2'] = dv * c.keep2.to(dtype) if c.keep2 is not None else dv
    for k, t in terms.items():
        o[k], o['abs_' + k] = (t * rows).sum(0), t.abs().sum(0)
    return o


def quantise(y, mut=()):
    """(bytes uint8, scale) of y [M, H] by the rule of the header, scale and the scaled row rounded to fp32 as the kernel holds them"""
    amax = y.abs().amax(-1).float()
    nz = amax > 0
    ys = torch.where(nz, amax / 448.0, torch.zeros_like(amax) if 'scale0' in mut else torch.ones_like(amax))
    inv = torch.where(nz, 448.0 / amax, torch.zeros_like(amax))
    return (y.float() * inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), ys.double()


def expected(c):
    """names of what a run of the case must deliver"""
    if c.kind == 'quant':
        return ('y8', 'ys')
    if c.kind == 'bwd':
        return ('dv',) + (('dv2',) if c.dv2 else ()) + tuple(SUM_CODE[k] for k in c.sums)
    if c.kind == 'fp8':
        return (('y',) if c.y else ()) + ('y8', 'ys', 'mean', 'rstd')
    if c.kind == 'sum':
        return ('y',) + c.outs + ('mean', 'rstd')
    return ('y', 'mean', 'rstd')


def store(c, vals, mut=()):
    """the values of compute() as the entry point's tensors hold them, in the form run() delivers (fp64; column sums started at 0.5)"""
    got = {}
    for k in expected(c):
        if k in T_OUT:
            got[k] = rb(vals[k]) if c.dt == 'bf16' else vals[k].float().double()
        elif k in F32_OUT:
            got[k] = vals[k].float().double()
        elif k in SUMS:
            got[k] = (vals[k].float() + 0.5).double()
    if 'y8' in expected(c):
        got['y8'], got['ys'] = quantise(vals['yq'], mut)
    return got


def reference(c):
    return compute(c, torch.float64)


def figures_of(c, ref):
    """the model (every output rounded once from the fp64 values) and the fp32 yardstick's maximum error per tensor"""
    f32 = compute(c, torch.float32)
    err = {k: float((f32[k].double() - ref[k]).abs().max()) for k in ref if not k.startswith('abs_')}
    return SimpleNamespace(model=store(c, ref), f32=err)


# ------------------------------------------------------------------ judging
def tile_rms(x, r):
    """relative RMS error per 16-row tile (the last one ragged), nan where the reference tile is all zero"""
    M = x.shape[0]
    pad = (-M) % 16
    e, n = ((x - r) ** 2).sum(-1), (r ** 2).sum(-1)
    if pad:
        z = torch.zeros(pad, dtype=e.dtype, device=e.device)
        e, n = torch.cat([e, z]), torch.cat([n, z])
    e, n = e.view(-1, 16).sum(-1), n.view(-1, 16).sum(-1)
    return torch.where(n > 0, torch.sqrt(e / n.clamp(min=1e-300)), torch.full_like(n, math.nan))


def f32_bound(c, ref, fig, k):
    src = 'yq' if k == 'yq' else k
    return max(4 * fig.f32[src], 2.0 ** -22 * float(ref[src].abs().max()))


def judge(c, got, ref, fig):
    """got: dict name -> fp64 tensor of the M rows (expected(c); y8 uint8).  Returns (figures, failures).  figures[x]: bf16 tensors (max error, the
    model's, tile RMS at the tile nearest its bound, the model's on that tile); fp32 tensors (max error, bound, worst error / bound); column sums
    (max error, worst error in units of 2^-24 (0.5 + sum |term|), that over C_SUM); y8 (max error of the dequantised value, worst error / bound);
    ys (max error, worst error / bound); masks 'keep' / 'keep2': (elements that differ from the host mask, 0, 0)."""
    m = fig.model
    figures, fails = {}, []
    missing = [x for x in expected(c) if x not in got]
    if missing:
        fails.append(f'missing: {missing}')
    for x in expected(c):
        if x not in got or x in ('y8', 'ys'):
            continue
        g = got[x]
        if not bool(torch.isfinite(g).all()):
            fails.append(f'{x}: non-finite')
            continue
        if x in SUMS:
            fp = 2.0 ** -24 * (0.5 + ref['abs_' + x])
            err = (g - 0.5 - ref[x]).abs()
            u = float((err / fp).max())
            if u > C_SUM:
                i = int((err / fp).argmax())
                fails.append(f'{x}: column {i} off by {float(err[i]):.3e} = {u:.3g} units of 2^-24 (0.5 + sum |term|), beyond {C_SUM:g}')
            figures[x] = (float(err.max()), u, u / C_SUM)
        elif x in T_OUT and c.dt == 'bf16':
            r, mo = ref[x], m[x]
            err, emax_m = (g - r).abs(), float((mo - r).abs().max())
            over = err - (2 * emax_m + A.ulp_bf16(r))
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
        else:
            b = f32_bound(c, ref, fig, x)
            err = (g - ref[x]).abs()
            if float(err.max()) > b:
                i = int(err.argmax())
                fails.append(f'{x}: element {i} off by {float(err.max()):.3e}, {float(err.max()) / b:.3g} x its fp32 bound {b:.3e}')
            figures[x] = (float(err.max()), b, float(err.max()) / b)
    if 'y8' in got and 'ys' in got:
        y = ref['yq']
        tight = 0.0 if c.kind == 'quant' else f32_bound(c, ref, fig, 'yq')
        amax = y.abs().amax(-1)
        zero = amax == 0
        want = torch.where(zero, torch.ones_like(amax), amax / 448)
        es = (got['ys'] - want).abs()
        lim_s = tight / 448 + 2.0 ** -23 * amax / 448
        if not bool(torch.isfinite(got['ys']).all()) or bool((es > lim_s).any()):
            i = int((es - lim_s).argmax())
            fails.append(f'ys: row {i} is {float(got["ys"][i]):.6e}, wanted {float(want[i]):.6e}')
        figures['ys'] = (float(es.max()), 0.0, float((es / lim_s.clamp(min=1e-300)).max()))
        deq = got['y8'].to(torch.uint8).view(torch.float8_e4m3fn).float().double() * got['ys'][:, None]
        err = (deq - y).abs()
        lim = 2.0 ** -4 * y.abs() * (1 + 2.0 ** -20) + 2.0 ** -10 * got['ys'][:, None] + tight
        lim = torch.where(zero[:, None], torch.zeros_like(lim), lim)               # a row of zeros: every byte 0, exactly
        bad = (err > lim) | (zero[:, None] & (got['y8'] != 0))
        if not bool(torch.isfinite(deq).all()) or bool(bad.any()):
            fails.append(f'y8: dequantised value {float((err / lim.clamp(min=1e-300)).max()):.3g} x its bound')
        figures['y8'] = (float(err.max()), 0.0, float((err / lim.clamp(min=1e-300))[~zero].max()) if bool((~zero).any()) else 0.0)
    for mk, out in (('keep', 'y' if c.kind != 'bwd' else None), ('keep2', 'dv2')):
        km = getattr(c, mk)
        if km is None or out is None or out not in got:
            continue
        live = ref[out] != 0 if mk == 'keep' else ref['dv'] != 0
        diff = int((((got[out] == 0) != (km == 0)) & (live | (km == 0))).sum())
        if diff:
            fails.append(f'{out}: {diff} elements zeroed where the host mask keeps them, or the reverse')
        figures[mk] = (float(diff), 0.0, 0.0)
    return figures, fails


# ------------------------------------------------------------------ running a case through an implementation (adapter4rec_amd._lib on the GPU, sim_lib on the CPU)
def _outbuf(c, W, dtype, sentinel, wide=None, rows=None):
    ld, c0 = _layout(W, c.wide if wide is None else wide)
    buf = torch.full((c.Mb if rows is None else rows, ld), sentinel, dtype=dtype, device=c.device)
    return buf, buf[:, c0:c0 + W], c0


def _intact(c, buf, c0, W, sentinel, nm):
    assert bool((buf[c.M:] == sentinel).all()), f'{c.name}: {nm} written at or beyond row M'
    assert bool((buf[:, :c0] == sentinel).all()) and bool((buf[:, c0 + W:] == sentinel).all()), f'{c.name}: {nm} written outside its columns'


def run(c, L):
    """the case through L's wrapper of its entry point; returns the dict judge takes, after the sentinel checks and the check that no input changed"""
    H, M, T, f32 = c.H, c.M, c.T, torch.float32
    before = {k: b.clone() for k, b in c.bufs.items()}
    o = {}
    gv = lambda nm: o[nm][1] if nm in o else None
    if c.kind != 'bwd' and c.kind != 'quant':
        o['stats'] = _outbuf(c, 2, f32, SENTINEL, 0)
    arena = None
    if c.kind == 'fwd':
        o['y'] = _outbuf(c, H, T, SENTINEL)
        L.ln_fwd(view(c, 'v'), c.gamma, c.beta, c.eps, gv('y'), gv('stats'), M=M, add=view(c, 'add')[:c.add_rows] if c.add_rows else None,
                 drop_p=c.drop, drop_site=c.drop_site, drop_seed=c.drop_seed)
    elif c.kind == 'fp8':
        if c.y:
            o['y'] = _outbuf(c, H, T, SENTINEL)
        o['y8'], o['ys'] = _outbuf(c, H, torch.uint8, SENTU8), _outbuf(c, 1, f32, SENTINEL, 0)
        L.ln_fwd(view(c, 'v'), c.gamma, c.beta, c.eps, gv('y'), gv('stats'), M=M, add=view(c, 'add')[:c.add_rows] if c.add_rows else None,
                 y8=gv('y8'), ys=o['ys'][0].view(-1))
    elif c.kind == 'quant':
        o['y8'], o['ys'] = _outbuf(c, H, torch.uint8, SENTU8), _outbuf(c, 1, f32, SENTINEL, 0)
        L.quant_rows_fp8(view(c, 'v'), gv('y8'), o['ys'][0].view(-1), M=M)
    elif c.kind == 'sum':
        o['y'] = _outbuf(c, H, T, SENTINEL)
        for nm in c.outs:
            o[nm] = _outbuf(c, H, T if nm == 'sum' else f32, SENTINEL)
        L.ln_fwd_sum(view(c, 'h'), None if c.res32 else view(c, 'res'), c.gamma, c.beta, c.eps, gv('y'), gv('stats'), M=M,
                     res32=view(c, 'res') if c.res32 else None, sum_out=gv('sum'), sum32=gv('sum32'), y32=gv('y32'))
    else:
        o['dv'] = _outbuf(c, H, T, SENTINEL)
        if c.dv2:
            o['dv2'] = _outbuf(c, H, T, SENTINEL)
        arena = torch.full((3 * (H + 8) + 8,), SENTINEL, dtype=f32, device=c.device)
        at = dict(dgamma=8, dbeta=H + 16, dbias=2 * H + 24)
        sums = {SUM_CODE[k]: arena[at[SUM_CODE[k]]:at[SUM_CODE[k]] + H] for k in c.sums}
        for t in sums.values():
            t.fill_(0.5)
        expect = arena.clone()
        L.ln_bwd(view(c, 'dy'), view(c, 'v'), view(c, 'stats'), c.gamma, gv('dv'), M=M, add=view(c, 'add')[:c.add_rows] if c.add_rows else None,
                 dgamma=sums.get('dgamma'), dbeta=sums.get('dbeta'), dbias=sums.get('dbias'), dres=view(c, 'dres') if c.dres else None,
                 drop_p=c.drop, drop_site=c.drop_site, drop_seed=c.drop_seed, dv2=gv('dv2'), drop2_p=c.drop2, drop2_site=c.drop2_site,
                 drop2_seed=c.drop2_seed)
    if c.device != 'cpu':
        torch.cuda.synchronize()
    for nm, (buf, vw, c0) in o.items():
        _intact(c, buf, c0, vw.shape[1], SENTU8 if buf.dtype == torch.uint8 else SENTINEL, nm)
    if arena is not None:
        keep = torch.ones_like(arena, dtype=torch.bool)
        for nm in sums:
            keep[at[nm]:at[nm] + H] = False
        assert torch.equal(arena[keep], expect[keep]), f'{c.name}: the neighbourhood of the sums (null pointers\' regions, gaps) was written'
    for k, b in before.items():
        assert torch.equal(b, c.bufs[k]), f'{c.name}: input {k} was written'
    got = {nm: o[nm][1][:M].double() for nm in o if nm not in ('stats', 'y8', 'ys')}
    if 'stats' in o:
        got['mean'], got['rstd'] = o['stats'][1][:M, 0].double(), o['stats'][1][:M, 1].double()
    if 'y8' in o:
        got['y8'], got['ys'] = o['y8'][1][:M].clone(), o['ys'][1][:M, 0].double()
    if arena is not None:
        got.update({nm: t.double() for nm, t in sums.items()})
    return got


# ------------------------------------------------------------------ the case table
WIDTHS = (8, 64, 504, 512, 520, 768, 1016, 1024)           # ng = H / 8: 1; 63 / 64 / 65 around the lane map's second group; 127 / 128
WIDTHS_QUANT = (8, 512, 520, 4088, 4096)                   # ng = 1, 64, 65, 511, 512 of the quantiser's 8-groups-per-lane layout
DTYPES = ('bf16', 'f32')
WALK_H = (72, 1024)
CASES = {}


def _add(name, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw, name=name, seed=900 + 13 * len(CASES))


def width_specs():
    """the width sweep at M = 37: forward lean and general, backward lean and general with all three sums, ln_fwd_sum, ln_fwd_fp8; the quantiser"""
    specs = []
    for di, dt in enumerate(DTYPES):
        for hi, H in enumerate(WIDTHS):
            w = (8, 64)[(hi + di) % 2]
            specs += [dict(name=f'w_fwd_lean_{dt}_H{H}', kind='fwd', H=H, M=37, dt=dt, wide=w),
                      dict(name=f'w_fwd_gen_{dt}_H{H}', kind='fwd', H=H, M=37, dt=dt, wide=72 - w, add_rows=20, drop=0.1),
                      dict(name=f'w_bwd_lean_{dt}_H{H}', kind='bwd', H=H, M=37, dt=dt, wide=72 - w, dres=hi % 2 == 0),
                      dict(name=f'w_bwd_gen_{dt}_H{H}', kind='bwd', H=H, M=37, dt=dt, wide=w, sums='gbv', dres=hi % 2 == 1, add_rows=20 if hi % 3 == 0 else 0),
                      dict(name=f'w_sum_{dt}_H{H}', kind='sum', H=H, M=37, dt=dt, wide=w, res32=hi % 2 == 0),
                      dict(name=f'w_fp8_{dt}_H{H}', kind='fp8', H=H, M=37, dt=dt, wide=72 - w, y=hi % 2 == 0)]
        for hi, H in enumerate(WIDTHS_QUANT):
            specs.append(dict(name=f'w_quant_{dt}_H{H}', kind='quant', H=H, M=37, dt=dt, wide=(8, 64)[(hi + di) % 2], cond='const'))
    return specs


def form_specs():
    """the forms at H = 72 (ng = 9) and M = 37 unless the form is about M: every <WGB, WDB>, one-sided dgamma / dbeta, the additive table's row
    counts, dropout forward and backward through the same mask, dv2, the optional outputs of ln_fwd_sum, ln_fwd_fp8 with and without y"""
    specs = []
    for dt in DTYPES:
        b = dict(H=72, M=37, dt=dt)
        for s in ('', 'g', 'b', 'gb', 'v', 'gv', 'bv', 'gbv'):                 # add keeps '' and the WGB-only forms on the general kernel at any M
            specs.append(dict(b, name=f'f_bwd_{dt}_sums_{s or "none"}', kind='bwd', sums=s, add_rows=20, dres=len(s) % 2 == 1, wide=(8, 64)[len(s) % 2]))
        for ar in (1, 20, 37, 40):
            specs.append(dict(b, name=f'f_fwd_{dt}_add{ar}', kind='fwd', add_rows=ar, wide=64))
            specs.append(dict(b, name=f'f_bwd_{dt}_add{ar}', kind='bwd', add_rows=ar, sums='gbv'))
        for p in (0.1, 0.5):
            specs.append(dict(b, name=f'f_fwd_{dt}_drop{p}', kind='fwd', drop=p, H=520))
            specs.append(dict(b, name=f'f_bwd_{dt}_drop{p}', kind='bwd', drop=p, H=520, sums='gbv', wide=64))
        specs.append(dict(b, name=f'f_bwd_{dt}_dv2', kind='bwd', dv2=True, drop2=0.1, dres=True, wide=64))
        specs.append(dict(b, name=f'f_bwd_{dt}_dv2_p0', kind='bwd', dv2=True, drop2=0.0, sums='v'))
        specs.append(dict(b, name=f'f_bwd_{dt}_dv2_both', kind='bwd', dv2=True, drop2=0.1, drop=0.1, sums='gb', dres=True, H=520))
        for i, outs in enumerate(((), ('sum',), ('sum32',), ('y32',), ('sum', 'sum32', 'y32'))):
            specs.append(dict(b, name=f'f_sum_{dt}_{"_".join(outs) or "none"}', kind='sum', outs=outs, res32=i % 2 == 0, wide=(8, 64)[i % 2]))
        specs.append(dict(b, name=f'f_sum_{dt}_res_all', kind='sum', res32=False))
        specs.append(dict(b, name=f'f_sum_{dt}_res32_all', kind='sum', res32=True, wide=64))
        for y in (False, True):
            specs.append(dict(b, name=f'f_fp8_{dt}_y{int(y)}', kind='fp8', y=y, add_rows=20 if y else 0, wide=(64, 8)[y]))
    return specs


def cond_specs():
    """conditioning: rows with mean >> spread, a constant row and a row of zeros, both eps"""
    specs = []
    for dt in DTYPES:
        for eps in (1e-6, 1e-12):
            e = f'{eps:g}'
            b = dict(H=768, M=37, dt=dt, eps=eps)
            specs += [dict(b, name=f'c_fwd_{dt}_offset_{e}', kind='fwd', cond='offset'),
                      dict(b, name=f'c_fwd_gen_{dt}_offset_{e}', kind='fwd', cond='offset', add_rows=1, wide=64),
                      dict(b, name=f'c_sum_{dt}_offset_{e}', kind='sum', cond='offset', res32=True),
                      dict(b, name=f'c_bwd_{dt}_offset_{e}', kind='bwd', cond='offset', sums='gbv', wide=64),
                      dict(b, name=f'c_fwd_{dt}_const_{e}', kind='fwd', cond='const', wide=64),
                      dict(b, name=f'c_bwd_{dt}_const_{e}', kind='bwd', cond='const', sums='gb'),
                      dict(b, name=f'c_fp8_{dt}_zero_{e}', kind='fp8', cond='zero')]
    return specs


def walk_specs(G):
    """the row-count walk; G = the CU count of the machine the kernels run on"""
    specs = []
    for dt in DTYPES:
        for H in WALK_H:
            b = dict(H=H, dt=dt)
            for M in (1, 3, 4, 5):                                        # around a workgroup's four waves
                specs.append(dict(b, name=f'r_fwd_lean_{dt}_H{H}_M{M}', kind='fwd', M=M))
                specs.append(dict(b, name=f'r_bwd_gen_{dt}_H{H}_M{M}', kind='bwd', M=M, sums='gbv', dres=True, wide=64))
            # 4096 + 5: the smallest M at which waves of the general backward carry sums over two rows under the 1024-block cap
            specs.append(dict(b, name=f'r_bwd_gen_{dt}_H{H}_M4101', kind='bwd', M=4096 + 5, sums='gbv'))
            for M in (8192 + 3, 3 * 8192 + 17):                           # 8192 = 4 rows x the largest resident grid: a second and a third row per wave
                specs.append(dict(b, name=f'r_fwd_lean_{dt}_H{H}_M{M}', kind='fwd', M=M, wide=64))
                specs.append(dict(b, name=f'r_fwd_gen_{dt}_H{H}_M{M}', kind='fwd', M=M, add_rows=20))
            for i, M in enumerate((2047, 2048, 2049, 8 * G + 1, 16 * G + 5)):  # the pg kernel: 2047 takes the general path
                M = M if i < 3 else max(M, PG_MIN_ROWS)
                for j, (dres, dv2, p2) in enumerate(((False, False, 0.0), (True, False, 0.0), (False, True, 0.0), (True, True, 0.1))):
                    specs.append(dict(b, name=f'r_bwd_pg_{dt}_H{H}_{("2047", "2048", "2049", "8G+1", "16G+5")[i]}_{("plain", "dres", "dv2p0", "dres_dv2")[j]}',
                                      kind='bwd', M=M, sums=('gb', 'g', 'b', 'gb')[(i + j) % 4], dres=dres, dv2=dv2, drop2=p2, wide=(8, 64)[(i + j) % 2]))
    return specs


# the cases of the CPU file by name, with fixed seeds: the width, form and conditioning tables as the GPU file runs them, and of the walk (G = 8)
# what decides a dispatch branch or a bound at sizes a CPU affords: the narrow width only beyond 5 rows, the two longest walks left to the GPU
for _s in width_specs() + form_specs() + cond_specs():
    _add(**_s)
for _s in walk_specs(8):
    if _s['M'] <= 5 or (_s['H'] == WALK_H[0] and _s['M'] <= 4101):
        _add(**_s)
_add('bwd_gen_bf16_H72_M4101_gbv_wide8', kind='bwd', H=72, M=4101, dt='bf16', sums='gbv', dres=True)


def seed_of(spec):
    """cases built at run time (sizes that depend on the CU count) take the seed of their name"""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(spec['name'])) % 100003


def names(prefix=''):
    return [n for n in CASES if n.startswith(prefix)]


def build(spec, device='cpu'):
    c = make_case(**dict(spec, seed=spec.get('seed', seed_of(spec))), device=device)
    c.ref = reference(c)
    c.fig = figures_of(c, c.ref)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its fp64 reference on the CPU, computed once per process and shared (read-only) by every test that needs it."""
    return build(CASES[name])


def colsum_ratio(c, ref, seed=0):
    """adapter_ln_ref.colsum_ratio's rule on a case of this file: the column sums in fp32 on the CPU, every term from the fp32 formulas, added one
    row after the other in a shuffled order onto 0.5: the worst |sum - (0.5 + ref)| / (2^-24 (0.5 + sum |term|)) per sum"""
    X = {k: t.float().cpu() for k, t in c.x.items()}
    x = X['v'] + (X['add'][torch.arange(c.M) % c.add_rows] if c.add_rows else 0)
    mean, rstd = X['stats'][:, 0:1], X['stats'][:, 1:2]
    xh = (x - mean) * rstd
    d = X['dy'] * c.keep.float().cpu() if c.keep is not None else X['dy']
    gm = d * X['gamma']
    dvln = rstd * (gm - gm.mean(-1, keepdim=True) - xh * (gm * xh).mean(-1, keepdim=True))
    terms = {k: t for k, t in dict(dgamma=d * xh, dbeta=d, dbias=dvln).items() if k in [SUM_CODE[s] for s in c.sums]}        # the sums the case is judged on
    perm = torch.randperm(c.M, generator=torch.Generator().manual_seed(seed)).tolist()
    out = {}
    for nm, t in terms.items():
        acc = torch.full((t.shape[1],), 0.5)
        for i in perm:
            acc += t[i]
        out[nm] = float(((acc.double() - 0.5 - ref[nm].cpu()).abs() / (2.0 ** -24 * (0.5 + ref['abs_' + nm].cpu()))).max())
    return out


def table_row(c, figures):
    """one line of the tables in the two test files' output: per tensor, worst error over bound (bf16 tensors: tile RMS over twice the model's and, in
    brackets, max error kernel / model; column sums: also in units u = 2^-24 (0.5 + sum |term|))"""
    row = f'{c.name:<44}{c.M:>6} {branch(c):<17}|'
    for x, f in figures.items():
        if len(f) == 4:
            row += f' {x} {f[2] / (2 * f[3]) if f[3] > 0 else f[2] / 2.0 ** -9:.2f} ({f[0]:.1e} / {f[1]:.1e})'
        elif x in SUMS:
            row += f' {x} {f[2]:.2f} ({f[1]:.2f} u)'
        elif x in ('keep', 'keep2'):
            row += f' {x} {int(f[0])} differ'
        else:
            row += f' {x} {f[2]:.2f} ({f[0]:.1e})'
    return row


def near_bound(figures, share=0.8):
    """the figures that came within 20 % of their bound"""
    out = []
    for x, f in figures.items():
        r = (f[2] / (2 * f[3]) if f[3] > 0 else f[2] / 2.0 ** -9) if len(f) == 4 else f[2]
        if r > share:
            out.append(x)
    return out
