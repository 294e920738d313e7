"""fp64 reference of the attention kernels (a4r_attn_fwd / _bwd: csrc/a4r_attn.hip, a4r_attn_small.hip; a4r_attn_long_fwd / _bwd:
csrc/a4r_attn_long.hip, a4r_attn_long.h, a4r_attn_long1.hip) and the cases their tests share.  TEST INFRASTRUCTURE ONLY.

forward_ref / backward_ref are plain torch and run on whichever device their inputs are on.  The backward is written out, not autograd:
    P~ = P keep ks      dV = P~^T dO      dP = (dO V^T) keep ks      delta = rowsum(P dP)      dS = P (dP - delta) scale      dQ = dS K      dK = dS^T Q
with ks = 1 / (1 - round(p 65536) / 65536), the kernels' a4r_keep_scale.

EXACT MASK.  The kernels add mask_neg to a disallowed score in fp32 (the long kernels replace it outright).  What that does, restated exactly:
  * a row with at least one allowed key gives its disallowed keys probability exactly 0 (exp underflows for every mask_neg in use);
  * mask_neg <= -1e9 (finfo(float32).min included): a row WITHOUT an allowed key is uniform, 1 / S over all S keys -- fp32 numbers near 1e9 are
    64 apart, so s + mask_neg rounds to mask_neg while |s| < 32 (SMAX; make_case asserts it for every case) -- and its dS = P (dP - delta) scale
    still reaches Q and K: the derivative of s + mask_neg with respect to s is 1.  An fp64 additive mask would keep s instead;
  * mask_neg = -10000 (K-Adapter blocks): s - 10000 is representable to one fp32 ulp at 1e4 = 2^-10, so in a row without an allowed key every
    score may move by 2^-10 against the row maximum's, a probability by the factor e^(2 * 2^-10) - 1 = 1.96e-3 < KAD_REL = 2e-3.  Such rows are
    judged at |out - ref| <= KAD_REL * (P~ |V|) (each probability off by at most that factor; bf16 adds its own roundings of P~ and of the stored
    value, 2^-9 each) and carry dO = 0, as behind the model's loss mask; rows
    with an allowed key are compared as everywhere else.

BOUNDS (judge).  fp32 instantiations: forward 1e-4, gradients 2e-4 (atol = rtol), lse 1e-3 -- the bounds tests/test_kernels_gpu.py holds them to,
here against fp64.  bf16: that file's elementwise bounds (3e-2 max(1, max |ref|) + 3e-2 |ref| forward, 4e-2 max |grad| + 3e-2 |ref| backward) AND,
per tensor, the relative RMS error per (item, head) and per (item, head, block of 16 rows = a query block / key tile of the kernels), each bounded by
twice the worst such figure of bf16_model on the same case (per (item, head) alone, one wrong row of 225 -- the last key tile dropped under a causal
mask -- dilutes below the bound: tests/test_attn_ref_cpu.py).  The model is fp64 arithmetic rounded to bf16 where the kernel sources round: P~ and dS before their MFMA (not in the scalar kernels for heads <= 16), the stored
out / dQ / dK / dV, and in the long kernels delta = dO . O taken from the stored (rounded) output.  The factor 2 covers accumulation order and the
exp2 path.  A model figure of exactly 0 (S = 1: P = 1) leaves only the store rounding: 2^-9.  A pair whose reference is all zero has no relative
figure; the elementwise bound covers it.
"""
import functools
import math
from types import SimpleNamespace

import torch

FMIN = torch.finfo(torch.float32).min
SMAX = 32.0
KAD_REL = 2e-3
SENTINEL = -768.0                       # exact in bf16 and fp32
JUNK = 777.0                            # what sits in gap columns / pad rows of the inputs: one such value read as data breaks every bound
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
TENSORS = ('out', 'dq', 'dk', 'dv')
PATTERNS = ('full', 'ragged', 'empty', 'left', 'holes', 'single')


def keep_scale(p):
    return 1.0 / (1.0 - round(p * 65536) / 65536.0) if p > 0 else 1.0


def rb(t):
    """round to bf16, back in fp64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


# ------------------------------------------------------------------ the reference
def forward_ref(q, k, v, allowed, scale, mask_neg, keepmul=None):
    """q, k, v [n, nh, S, dh]; allowed None or bool, broadcastable to [n, nh, S, S]; keepmul None or keep * ks [n, nh, S, S].
    Returns out [n, nh, S, dh], lse [n, nh, S] (over the allowed keys; log S in a row without one), P and P~."""
    s = (q @ k.transpose(-1, -2)) * scale
    if allowed is None:
        x = s
    elif mask_neg <= -1e9:
        x = torch.where(allowed, s, torch.full_like(s, -math.inf))
        x = torch.where(allowed.any(-1, keepdim=True), x, torch.zeros_like(s))
    else:
        x = torch.where(allowed, s, s + mask_neg)
    lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse[..., None])
    pt = p if keepmul is None else p * keepmul
    return pt @ v, lse, p, pt


def backward_ref(q, k, v, do, p, scale, keepmul=None):
    km = 1.0 if keepmul is None else keepmul
    dv = (p * km).transpose(-1, -2) @ do
    dp = (do @ v.transpose(-1, -2)) * km
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    return ds @ k, ds.transpose(-1, -2) @ q, dv


def bf16_model(q, k, v, do, p, scale, keepmul=None, round_p=True, delta_from_out=False):
    """The same step with the kernels' bf16 roundings (see the header): out, dq, dk, dv."""
    km = 1.0 if keepmul is None else keepmul
    r = rb if round_p else (lambda t: t)
    pt = r(p * km)
    out = rb(pt @ v)
    dv = rb(pt.transpose(-1, -2) @ do)
    dp = (do @ v.transpose(-1, -2)) * km
    delta = (do * out).sum(-1, keepdim=True) if delta_from_out else (p * dp).sum(-1, keepdim=True)
    ds = r(p * (dp - delta))
    return out, rb(ds @ k * scale), rb(ds.transpose(-1, -2) @ q * scale), dv


# ------------------------------------------------------------------ masks
def pattern_row(name, S):
    m = torch.zeros(S)
    if name == 'full':
        m[:] = 1
    elif name == 'ragged':                       # a title shorter than S: pad keys on the right
        m[:max(1, S // 2)] = 1
    elif name == 'left':                         # a short history: pad keys on the left
        m[min(3, S - 1):] = 1
    elif name == 'holes':
        m[::3] = 1
    elif name == 'single':
        m[S // 3] = 1
    return m                                     # 'empty': the all-PAD item


def key_mask_of(n_items, S):
    return torch.stack([pattern_row(PATTERNS[i % len(PATTERNS)], S) for i in range(n_items)])


def allowed_of(km, S, causal, device=None):
    """bool [n, 1, S, S] or None"""
    if km is None and not causal:
        return None
    a = torch.ones(1, 1, S, S, dtype=torch.bool, device=device)
    if causal:
        a = torch.tril(a)
    if km is not None:
        a = a & (km.to(device) != 0)[:, None, None, :]
    return a


# ------------------------------------------------------------------ cases
def make_case(name, family, dt, dh, S, nh, n_items, causal=False, mask=None, neg=-1e9, drop=0.0, lens=None, seed=0, device='cpu'):
    """family 'short' (a4r_attn_*) or 'long' (a4r_attn_long_*); mask None or 'all6' (item i carries PATTERNS[i % 6]); lens: packed items.
    The buffers, as the kernels get them: qkv [rows, ld] with the blocks in the order v, q, k, an 8-element gap behind each (ld = 3 Hd + 24), out /
    dout [rows, ldo = Hd + 8]; every offset a multiple of 16 bytes; rows padded to 128 (short) / 256 (long); gaps and pad rows hold JUNK."""
    t = DT[dt]
    Hd = nh * dh
    g = torch.Generator().manual_seed(seed)
    off = dict(v=0, q=Hd + 8, k=2 * Hd + 16)
    ld, ldo = 3 * Hd + 24, Hd + 8
    if lens is not None:
        lens_t = torch.tensor(lens)
        row0 = torch.cumsum(lens_t, 0) - lens_t
    else:
        lens_t = torch.full((n_items,), S)
        row0 = torch.arange(n_items) * S
    n_rows = int(lens_t.sum())
    pad = 128 if family == 'short' else 256
    Mp = (n_rows + pad - 1) // pad * pad + pad                       # (always at least one whole block of pad rows)
    pos = torch.arange(S)
    valid = pos[None, :] < lens_t[:, None]                           # [n, S]
    rows = (row0[:, None] + pos[None, :]).clamp(max=n_rows - 1)      # buffer row of (item, position)
    vr = rows[valid]
    qkv = torch.full((Mp, ld), JUNK)
    dout = torch.full((Mp, ldo), JUNK)
    for o in off.values():
        qkv[:n_rows, o:o + Hd] = torch.randn(n_rows, Hd, generator=g)
    dout[:n_rows, :Hd] = torch.randn(n_rows, Hd, generator=g)
    qkv, dout = qkv.to(t), dout.to(t)                                # bf16 cases: the inputs ARE bf16 numbers
    km = key_mask_of(n_items, S) if mask == 'all6' else None
    c = SimpleNamespace(name=name, family=family, dt=dt, t=t, dh=dh, S=S, nh=nh, n_items=n_items, Hd=Hd, causal=causal, mask=mask, neg=neg, drop=drop,
                        lens=lens, seed=seed, off=off, ld=ld, ldo=ldo, n_rows=n_rows, Mp=Mp, valid=valid, rows=rows, km=km, scale=1.0 / math.sqrt(dh),
                        drop_site=16 + seed % 7, drop_seed=0x5eed * 1000003 + seed, offsets=None)
    if lens is not None:
        c.offsets = torch.cat([row0, torch.tensor([n_rows])]).to(torch.int32)
    allowed = allowed_of(km, S, causal)
    if lens is not None:                                              # packed: item i is evaluated on its own lens[i] tokens
        allowed = (allowed if allowed is not None else torch.ones(1, 1, S, S, dtype=torch.bool)) & valid[:, None, None, :]
    c.allowed = allowed
    c.any_key = torch.ones(n_items, S, dtype=torch.bool) if allowed is None else allowed.any(-1)[:, 0].expand(n_items, S).clone()
    if neg > -1e9:                                                    # rows without an allowed key carry no gradient (see the header)
        d = dout[:n_rows, :Hd].clone()
        d[vr] = d[vr] * c.any_key[valid].to(t)[:, None]
        dout[:n_rows, :Hd] = d
    c.qkv, c.dout = qkv.to(device), dout.to(device)
    c.key_mask = km.to(device) if km is not None and lens is None else None       # (packed items: the kernels ignore the key mask)
    c.q, c.k, c.v = (gather(c, c.qkv, off[x]) for x in 'qkv')
    c.do = gather(c, c.dout, 0)
    c.keepmul = None
    if drop > 0:
        c.keepmul = keep_multiplier(c, c.drop_site).to(device)
    smax = float(((c.q @ c.k.transpose(-1, -2)) * c.scale).abs().max())
    assert smax < SMAX, (name, smax)
    c.smax = smax
    return c


def keep_multiplier(c, site):
    from oracle.dropout_masks import DropoutStream
    m = DropoutStream(c.drop_seed).mask('attn_item', site, torch.empty(c.n_items, c.nh, c.S, c.S), c.drop, head_dim=c.dh, long_kernels=c.family == 'long')
    return (m > 0).to(torch.float64) * keep_scale(c.drop)


def gather(c, buf, col):
    """[rows, ld] buffer -> fp64 [n, nh, S, dh] (positions a packed item does not have: zero)"""
    x = buf[c.rows.to(buf.device).reshape(-1), col:col + c.Hd].to(torch.float64).view(c.n_items, c.S, c.nh, c.dh)
    return (x * c.valid.to(buf.device)[:, :, None, None]).transpose(1, 2).contiguous()


def reference(c, allowed='case', keepmul='case', k=None):
    """fp64 out, lse, p, dq, dk, dv of the case (the keyword arguments let the mutation checks swap one ingredient)."""
    dev = c.q.device
    allowed = c.allowed if isinstance(allowed, str) else allowed
    keepmul = c.keepmul if isinstance(keepmul, str) else keepmul
    k = c.k if k is None else k
    a = allowed.to(dev) if allowed is not None else None
    out, lse, p, _ = forward_ref(c.q, k, c.v, a, c.scale, c.neg, keepmul)
    dq, dk, dv = backward_ref(c.q, k, c.v, c.do, p, c.scale, keepmul)
    r = SimpleNamespace(out=out, lse=lse, p=p, dq=dq, dk=dk, dv=dv)
    if c.lens is not None:                                            # positions an item does not have
        vq = c.valid.to(dev)[:, None, :, None]
        for x in TENSORS:
            setattr(r, x, getattr(r, x) * vq)
    return r


def model_figures(c, ref):
    """worst relative RMS error of bf16_model per tensor, (per (item, head), per 16-row block of one): what judge holds a bf16 kernel to, times two"""
    m = bf16_model(c.q, c.k, c.v, c.do, ref.p, c.scale, c.keepmul, round_p=c.dh > 16, delta_from_out=c.family == 'long')
    fig = {}
    for x, got in zip(TENSORS, m):
        fig[x] = tuple(_worst(pair_rms(c, x, got, getattr(ref, x), rows)) for rows in (None, 16))
    return fig


# ------------------------------------------------------------------ judging
def _rows_judged(c, x, dev):
    """[n, 1, S, 1] bool: the rows of tensor x that the ordinary bounds look at (all but the -10000 rows without an allowed key, in out)"""
    m = c.valid.to(dev)
    if x == 'out' and c.neg > -1e9:
        m = m & c.any_key.to(dev)
    return m[:, None, :, None]


def pair_rms(c, x, got, ref, rows=None):
    """[n, nh] relative RMS error per (item, head) -- rows=16: [n, nh, ceil(S / 16)], per block of 16 rows, the kernels' query block / key tile --;
    nan where the reference is all zero"""
    m = _rows_judged(c, x, ref.device).to(ref.dtype)
    e, r = (((got - ref) * m) ** 2).sum(-1), ((ref * m) ** 2).sum(-1)
    if rows is None:
        e, r = e.sum(-1), r.sum(-1)
    else:
        nb = (c.S + rows - 1) // rows
        fold = lambda t: torch.nn.functional.pad(t, (0, nb * rows - c.S)).view(*t.shape[:-1], nb, rows).sum(-1)
        e, r = fold(e), fold(r)
    return torch.where(r > 0, torch.sqrt(e / r.clamp(min=1e-300)), torch.full_like(r, math.nan))


def _worst(f):
    ok = ~torch.isnan(f)
    return float(f[ok].max()) if bool(ok.any()) else math.nan


def judge(c, got, ref, fig=None):
    """got: a namespace / dict with out, dq, dk, dv [n, nh, S, dh] (any float dtype).  Returns (figures, failures): figures[x] = (max abs error,
    worst error / bound, worst pair RMS); failures = the list of bounds missed.  fig: model_figures of the case (bf16 cases)."""
    get = (lambda x: got[x]) if isinstance(got, dict) else (lambda x: getattr(got, x))
    figures, fails = {}, []
    gmax = max(float(getattr(ref, x).abs().max()) for x in ('dq', 'dk', 'dv'))
    for x in TENSORS:
        g, r = get(x).to(torch.float64), getattr(ref, x)
        if not bool(torch.isfinite(g).all()):
            fails.append(f'{x}: non-finite')
            figures[x] = (math.inf, math.inf, math.inf)
            continue
        if c.t == torch.float32:
            atol = rtol = 1e-4 if x == 'out' else 2e-4
        else:
            atol, rtol = (3e-2 * max(1.0, float(r.abs().max())) if x == 'out' else 4e-2 * gmax), 3e-2
        m = _rows_judged(c, x, r.device)
        err = (g - r).abs() * m
        ratio = float((err / (atol + rtol * r.abs())).max())
        if ratio > 1:
            fails.append(f'{x}: elementwise {ratio:.3g} x bound (max err {float(err.max()):.3e})')
        worst = math.nan
        if x == 'out' and c.neg > -1e9:                                   # rows without an allowed key under -10000 (see the header)
            mk = (c.valid & ~c.any_key).to(r.device)[:, None, :, None]
            pv = (ref.p if c.keepmul is None else ref.p * c.keepmul) @ c.v.abs()
            if c.t == torch.float32:
                lim = KAD_REL * pv
            else:          # bf16: P~ is rounded before its MFMA (2^-9 each; not in the scalar kernels) and so is the stored value (2^-9 of what is stored)
                lim = (KAD_REL + (2.0 ** -9 if c.dh > 16 else 0.0)) * pv
                lim = lim * (1 + 2.0 ** -9) + 2.0 ** -9 * r.abs()
            bad = ((g - r).abs() > lim + 1e-6) & mk
            if bool(bad.any()):
                fails.append(f'{x}: {int(bad.sum())} values of rows without an allowed key beyond {KAD_REL} relative')
        for gi, (rows, what) in enumerate(((None, '(item, head)'), (16, '(item, head, 16-row block)'))):
            pr = pair_rms(c, x, g, r, rows)
            w = _worst(pr)
            if gi == 0:
                worst = w
            if c.t == torch.bfloat16 and fig is not None and not math.isnan(w):
                mf = fig[x][gi]
                lim = 2.0 * mf if mf > 0 else 2.0 ** -9
                if w > lim:
                    i = int(torch.nan_to_num(pr, nan=-1.0).argmax())
                    fails.append(f'{x}: relative RMS {w:.3e} of {what} {tuple(int(v) for v in torch.unravel_index(torch.tensor(i), pr.shape))} beyond {lim:.3e} = 2 x the bf16 model')
        figures[x] = (float(err.max()), ratio, worst)
    return figures, fails


# ------------------------------------------------------------------ the case table (the CPU file proves it sound, the GPU file runs it)
CASES = {}
SHORT_COMBOS = [('f32', 8), ('bf16', 8), ('f32', 16), ('bf16', 16), ('f32', 32), ('bf16', 32), ('f32', 64), ('bf16', 64), ('f32', 128), ('f32', 256)]
SHORT_S = (1, 2, 15, 16, 17, 31, 32)
LONG_COMBOS = [('f32', 64), ('bf16', 64), ('f32', 32), ('bf16', 32)]
LONG_EDGES = (1, 32, 33, 64, 65, 128, 129, 224, 225, 256)                 # low and high edge of each of nkt_for's five instantiations
LONG_INNER = (16, 17, 144, 145, 161, 193, 209, 241)
ONEPASS_S = (129, 144, 145, 161, 193, 209, 224)
NEGS = (FMIN, -1e9, -10000.0)


def kernel_family(dh):
    return 'scalar' if dh <= 16 else 'wide' if dh >= 128 else 'mfma'


def _add(name, **kw):
    assert name not in CASES, name
    CASES[name] = dict(kw, name=name, seed=1000 + 7 * len(CASES))


# short kernels: every S with every (type, head width); the other axes cycle so that every value meets every kernel family (the CPU file asserts it).
# 7 items x 3 or 1 heads = 21 / 7 pairs: no multiple of the 4, 2, 1 waves (scalar kernels: 2 pairs) of a workgroup.
for ci, (dt_, dh_) in enumerate(SHORT_COMBOS):
    for si, S_ in enumerate(SHORT_S):
        i = ci * len(SHORT_S) + si
        j = si + ci // 2                                             # (ci // 2: both types of a width take the same turn)
        _add(f'short_{dt_}_dh{dh_}_S{S_}', family='short', dt=dt_, dh=dh_, S=S_, nh=(3, 1)[(j // 2) % 2], n_items=7, causal=bool(j % 2),
             mask=None if j % 4 == 3 else 'all6', neg=NEGS[(si + ci) % 3], drop=(0.0, 0.25)[(si + ci // 2 + ci // 4) % 2])
for ci, (dt_, dh_) in enumerate([('f32', 32), ('bf16', 32), ('f32', 64), ('bf16', 64)]):      # packed items, one per MFMA kernel
    _add(f'packed_{dt_}_dh{dh_}', family='short', dt=dt_, dh=dh_, S=32, nh=3, n_items=7, lens=(32, 1, 17, 16, 15, 31, 2), drop=(0.0, 0.25)[ci // 2 ^ ci % 2])
# long kernels
for ei, S_ in enumerate(LONG_EDGES):
    for ci, (dt_, dh_) in enumerate(LONG_COMBOS):
        nh_ = (2, 3, 1)[(ei + ci) % 3]
        _add(f'long_{dt_}_dh{dh_}_S{S_}', family='long', dt=dt_, dh=dh_, S=S_, nh=nh_, n_items=3 + (ei + ci) % 3)
        _add(f'long_{dt_}_dh{dh_}_S{S_}_key', family='long', dt=dt_, dh=dh_, S=S_, nh=nh_, n_items=6, mask='all6', neg=FMIN)
        _add(f'long_{dt_}_dh{dh_}_S{S_}_causal', family='long', dt=dt_, dh=dh_, S=S_, nh=nh_, n_items=6, mask='all6', causal=True, neg=(-1e9, FMIN)[(ei + ci) % 2])
for si, S_ in enumerate(LONG_INNER):                                     # the lengths inside: one fp32 and one bf16 instantiation each
    for dt_, dh_ in (('f32', (64, 32)[si % 2]), ('bf16', (32, 64)[si % 2])):
        _add(f'long_{dt_}_dh{dh_}_S{S_}', family='long', dt=dt_, dh=dh_, S=S_, nh=2, n_items=5)
for S_ in ONEPASS_S:                                                     # bf16, head width 64, no mask, 129 .. 224: the one-pass backward by default
    if f'long_bf16_dh64_S{S_}' not in CASES:
        _add(f'long_bf16_dh64_S{S_}', family='long', dt='bf16', dh=64, S=S_, nh=2, n_items=5)
    _add(f'long_bf16_dh64_S{S_}_drop', family='long', dt='bf16', dh=64, S=S_, nh=3, n_items=5, drop=0.25)
for S_ in (17, 33, 65, 128):                                             # head width 128 (fp32, up to 128 tokens)
    _add(f'long_f32_dh128_S{S_}', family='long', dt='f32', dh=128, S=S_, nh=1 + S_ % 2, n_items=5)
    _add(f'long_f32_dh128_S{S_}_causal', family='long', dt='f32', dh=128, S=S_, nh=2, n_items=6, mask='all6', causal=True, neg=-1e9)
for S_ in (17, 33, 65, 145, 241):                                        # dropout: one length per instantiation
    for dt_, dh_ in LONG_COMBOS + ([('f32', 128)] if S_ <= 65 else []):
        if f'long_{dt_}_dh{dh_}_S{S_}_drop' not in CASES:
            _add(f'long_{dt_}_dh{dh_}_S{S_}_drop', family='long', dt=dt_, dh=dh_, S=S_, nh=2, n_items=3, drop=0.25)


def names(prefix, **where):
    return [n for n, s in CASES.items() if n.startswith(prefix) and all(s.get(k_, None) == v_ for k_, v_ in where.items())]


def walk_spec(cu, S, drop):
    """The persistent walk of the one-pass backward (min(pairs, CU count) workgroups, stride = the grid): bf16, head width 64, 3 heads and as many
    items as put the pair count at 2.5 x the CU count -- every workgroup serves two or three pairs, both LDS image sets are reused."""
    n_items = (5 * cu) // 6
    return dict(name=f'walk_cu{cu}_S{S}_drop{int(drop > 0)}', family='long', dt='bf16', dh=64, S=S, nh=3, n_items=n_items, drop=drop, seed=4242 + S)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its fp64 reference on the CPU, computed once per process and shared (read-only) by every test that needs it."""
    c = make_case(**CASES[name])
    c.ref = reference(c)
    c.fig = model_figures(c, c.ref) if c.t == torch.bfloat16 else None
    return c
