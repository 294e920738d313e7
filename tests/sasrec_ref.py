"""fp64 reference of the one-launch SASRec block (a4r_sasrec_block_fwd / _bwd) and the cases its tests share.  TEST INFRASTRUCTURE ONLY.

block_ref() restates the block from the header comment of adapter4rec_amd/csrc/a4r_sasrec.hip in plain torch on the CPU, without sim_lib:
    h   = dropout(ctx W_fc^T)                 ctx = dropout(softmax(Q K^T / sqrt(dh), masked)) V      (2 heads x 32)
    mode 0:  x1 = LN1(x + A1(h));  y = LN2(x1 + A2(dropout(relu(x1 W1^T + b1) W2^T + b2)))           A(h) = act(h Wd^T + bd) Wu^T + bu [+ h]
    mode 1:  x1 = LN1(x + h);  va = dropout(relu(x1 W1^T + b1) W2^T + b2) + x1;  y = LN3(A2(LN2(va)) + va)      (Pfeiffer: A2 has no inner residual)

Two things differ from evaluating sim_lib._sasrec_block_fn in fp64:
  * MASK.  A disallowed score (key padded, key > query, key >= T) is EXACTLY mask_neg, not s + mask_neg.  The kernel computes s + mask_neg in
    fp32, where the spacing of numbers near 1e9 is 64: the sum rounds to mask_neg whenever |s| < 32, so a fully padded query row attends
    uniformly over its T keys.  fp64 would keep s.  block_ref returns smax = max |s / sqrt(dh)| so that callers can assert smax < 32, the
    condition under which this reference describes the kernel.  The DERIVATIVE of a masked score with respect to s stays 1, as autograd
    has it for `s + mask_neg` and as the kernel's dS = P (dP - sum P dP) has it: it matters only in a fully padded row, the one place
    where masked keys carry probability.
  * DROPOUT.  `masks` holds the multipliers (0 or 1 / (1 - p)) of oracle/dropout_masks.py's DropoutStream(seed, sasrec_fused=True) at the
    kernel's three sites: the probabilities [users, 2, T, T] ('attn_user', site), h after the W_fc product ('rows_user', site + 1) and
    h2 after W2 + b2 ('rows_user', site + 2).

KINKS.  The block's gradient is discontinuous where a ReLU (or leaky ReLU) input crosses zero: a pre-activation that fp32 and fp64 put on
different sides of zero moves gradient entries by O(0.1) although both evaluations are right.  block_ref returns the fp64 pre-activations
of every kinked site; a user is "near a kink" when one of them is below KINK = 1e-5 in magnitude (ten times the ~1e-6 fp32 error of a
pre-activation of order 1).  Cases of at most 8 users use seeds without such a user; the 600-user cases zero dy for those users (they
then contribute exactly nothing to any gradient on either side), at most KINK_CAP of the users.  tests/test_sasrec_ref_cpu.py asserts
all of this for every case below, on the CPU.
"""
import functools
import math
from types import SimpleNamespace

import torch

E, NH, DH, F = 64, 2, 32, 256
KINK = 1e-5                  # |pre-activation| below this: the user is near a kink
KINK_CAP = 0.10              # at most this share of a many-user case may have dy zeroed
SMAX = 32.0                  # |scaled score| below this: fp32 s + mask_neg == mask_neg for mask_neg = -1e9
ADAPTER_GRADS = ('wd1', 'bd1', 'wu1', 'bu1', 'wd2', 'bd2', 'wu2', 'bu2')


def dpe_of(d):
    """The kernel's adapter width in LDS: d rounded up to the 16-column MFMA tile."""
    return (d + 15) & ~15


def grad_names(mode):
    """Trainable tensors of the block: mode 1 carries no adapter on the attention sub-layer but a trainable LN3."""
    return ('wd2', 'bd2', 'wu2', 'bu2', 'ln3_g', 'ln3_b') if mode == 1 else ADAPTER_GRADS


def _act(x, a):
    if a == 1:
        return torch.relu(x)
    if a == 2:
        return torch.nn.functional.gelu(x)
    if a == 3:
        return torch.nn.functional.gelu(x, approximate='tanh')
    if a == 4:
        return torch.nn.functional.leaky_relu(x, 0.01)
    return x


def block_ref(desc, x, log_mask, T, dy=None, masks=None, dtype=torch.float64):
    """desc: the a4r_sasrec_block_t fields as CPU tensors (Wd [>= d rows, 64], bd [>= d], Wu [64, ldwu]: only the first d rows / columns are
    read); x [B * T, 64]; log_mask [B, T] (non-zero = a real item); masks: None or dict(attn [B, 2, T, T], h [B, T, 64], h2 [B, T, 64]).
    Returns a namespace: y [B * T, 64], smax, pre (dict: 'ffn' [B, T, 256] and, where act is ReLU / leaky ReLU, 'ad1' / 'ad2' [B, T, d]) and,
    given dy, dx [B * T, 64] and grads (dict over grad_names(mode), compact: wd [d, 64], bd [d], wu [64, d], bu [64])."""
    c = lambda t: t.detach().to(dtype)
    B = x.shape[0] // T
    d, act, mode = desc['d'], desc['act'], desc.get('mode', 0)
    inner = bool(desc['inner_res']) and mode == 0
    W = {k: c(desc[k]) for k in ('wqkv', 'wfc', 'w1', 'b1', 'w2', 'b2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b')}
    A = {}
    for k in ('1', '2'):
        A['wd' + k], A['bd' + k] = c(desc['wd' + k])[:d].clone(), c(desc['bd' + k])[:d].clone()
        A['wu' + k], A['bu' + k] = c(desc['wu' + k])[:, :d].clone(), c(desc['bu' + k]).clone()
    if mode == 1:
        A['ln3_g'], A['ln3_b'] = c(desc['ln3_g']).clone(), c(desc['ln3_b']).clone()
    names = grad_names(mode)
    xin = c(x).view(B, T, E).clone()
    if dy is not None:
        xin.requires_grad_(True)
        for k in names:
            A[k].requires_grad_(True)
    mk = (lambda k: masks[k].to(dtype)) if masks is not None else None
    pre = {}

    def ln(v, g, b):
        mu = v.mean(-1, keepdim=True)
        return (v - mu) * torch.rsqrt(((v - mu) ** 2).mean(-1, keepdim=True) + desc['eps']) * g + b

    def adapter(hh, k, res):
        zp = hh @ A['wd' + k].t() + A['bd' + k]
        if act in (1, 4):
            pre['ad' + k] = zp.detach()
        return _act(zp, act) @ A['wu' + k].t() + A['bu' + k] + (hh if res else 0)

    with torch.enable_grad() if dy is not None else torch.no_grad():
        qkv = xin @ W['wqkv'].t()
        q, k_, v = (t.view(B, T, NH, DH).transpose(1, 2) for t in qkv.split(E, dim=-1))
        s = (q @ k_.transpose(-1, -2)) / math.sqrt(DH)
        smax = float(s.detach().abs().max())
        allowed = (log_mask[:, None, None, :] != 0) & torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None]
        s = torch.where(allowed, s, (s - s.detach()) + desc['mask_neg'])           # exactly mask_neg, derivative 1 (see the header)
        p = torch.softmax(s, -1)
        if mk:
            p = p * mk('attn')
        h = (p @ v).transpose(1, 2).reshape(B, T, E) @ W['wfc'].t()
        if mk:
            h = h * mk('h')
        x1 = ln(xin + (h if mode == 1 else adapter(h, '1', inner)), W['ln1_g'], W['ln1_b'])
        u = x1 @ W['w1'].t() + W['b1']
        pre['ffn'] = u.detach()
        h2 = torch.relu(u) @ W['w2'].t() + W['b2']
        if mk:
            h2 = h2 * mk('h2')
        if mode == 1:
            va = h2 + x1
            y = ln(adapter(ln(va, W['ln2_g'], W['ln2_b']), '2', False) + va, A['ln3_g'], A['ln3_b'])
        else:
            y = ln(x1 + adapter(h2, '2', inner), W['ln2_g'], W['ln2_b'])
        out = SimpleNamespace(y=y.detach().reshape(B * T, E), smax=smax, pre=pre, dx=None, grads=None)
        if dy is not None:
            g = torch.autograd.grad(y, [xin] + [A[k] for k in names], c(dy).view(B, T, E))
            out.dx = g[0].reshape(B * T, E)
            out.grads = dict(zip(names, g[1:]))
    return out


def near_kink_users(pre, thr=KINK):
    """bool [B]: users with a kinked pre-activation of magnitude below thr."""
    bad = None
    for v in pre.values():
        b = (v.abs() < thr).flatten(1).any(1)
        bad = b if bad is None else bad | b
    return bad


def dropout_multipliers(seed, site, B, T, p_attn, p_hidden):
    """The block's three masks as the kernel draws them (a4r_sasrec.hip: probabilities, h, h2)."""
    from oracle.dropout_masks import DropoutStream
    st = DropoutStream(seed, sasrec_fused=True)
    return dict(attn=st.mask('attn_user', site, torch.empty(B, NH, T, T), p_attn),
                h=st.mask('rows_user', site + 1, torch.empty(B, T, E), p_hidden),
                h2=st.mask('rows_user', site + 2, torch.empty(B, T, E), p_hidden))


def make_case(B, T, d, ldwu=64, ldg_d=64, ldg_u=64, mode=0, act=1, inner=True, pads=None, seed=0, pad_fill=0.0,
              drop_attn=0.0, drop_hidden=0.0, drop_seed=1234567, drop_site=4096):
    """(desc, x, log_mask, dy) on the CPU.  pads: left padding per user (a tuple, or 'cycle': user u has u % (T + 1) padded positions, so
    every padding length including the fully padded user occurs).  pad_fill: scale of the values in rows d.. of Wd / bd and columns d.. of
    Wu.  The engine keeps them zero (include/a4r.h); the kernel masks columns >= d itself, so a non-zero fill checks that no tile reads them."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    dpe = dpe_of(d)
    desc = dict(wqkv=r(192, 64, sc=0.15), wfc=r(64, 64, sc=0.15), w1=r(256, 64, sc=0.15), b1=r(256, sc=0.1), w2=r(64, 256, sc=0.08), b2=r(64, sc=0.1),
                ln1_g=1 + r(64, sc=0.1), ln1_b=r(64, sc=0.1), ln2_g=1 + r(64, sc=0.1), ln2_b=r(64, sc=0.1),
                E=64, n_heads=2, F=256, d=d, ldwu=ldwu, ldg_d=ldg_d, ldg_u=ldg_u, act=act, inner_res=int(inner), eps=1e-6, mask_neg=-1e9,
                drop_attn=drop_attn, drop_hidden=drop_hidden, drop_site=drop_site, drop_seed=drop_seed, mode=mode)
    for k in ('1', '2'):
        wd, wu, bd = r(dpe, 64, sc=pad_fill), r(64, ldwu, sc=pad_fill), r(dpe, sc=pad_fill)
        wd[:d], wu[:, :d], bd[:d] = r(d, 64, sc=0.2), r(64, d, sc=0.2), r(d, sc=0.1)
        desc.update({'wd' + k: wd, 'bd' + k: bd, 'wu' + k: wu, 'bu' + k: r(64, sc=0.1)})
    if mode == 1:
        desc.update(ln3_g=1 + r(64, sc=0.1), ln3_b=r(64, sc=0.1))
    x, dy = r(B * T, 64), r(B * T, 64)
    mask = torch.ones(B, T)
    for u in range(B):
        mask[u, :(u % (T + 1) if pads == 'cycle' else pads[u])] = 0
    return desc, x, mask, dy


# ------------------------------------------------------------------ the cases (one list: the CPU file proves them sound, the GPU file runs them)
def _pads6(T):
    """Six users whose left padding includes 0, 1, T - 1 and T (fully padded)."""
    return (0, min(1, T), T - 1, T, T // 2, 0)


CASES = {}


def _add(group, name, **kw):
    kw.setdefault('B', 6)
    kw.setdefault('pads', _pads6(kw['T']) if kw['B'] == 6 else 'cycle')
    CASES[name] = dict(kw, group=group, seed=SEEDS.get(name, 1000 + 7 * len(CASES)))


# Seeds of the cases whose default seed (1000 + 7 * position) has a user near a kink: the next seed without one.
SEEDS = {'T17': 1029, 'T32_d15_ldwu64': 1071, 'T32_d16_ldwu16': 1078, 'T17_d1_ldwu16': 1120, 'mode0_inner1_act3': 1211, 'mode0_inner0_act3': 1246,
         'mode1_inner0_act2': 1274, 'drop_T17_mode1_both': 1331, 'drop_T17_mode1_hidden': 1344}

for T_ in (1, 2, 15, 16, 17, 31, 32):                                  # every row-tile split of the 32 padded rows
    _add('T', f'T{T_}', T=T_, d=16)
for T_ in (32, 17):                                                    # adapter widths on every side of the 16-column tile; compact leading dimensions
    for d_ in (1, 15, 16, 17, 32):
        for ld_ in sorted({dpe_of(d_), 64}):
            _add('d', f'T{T_}_d{d_}_ldwu{ld_}', T=T_, d=d_, ldwu=ld_, ldg_d=68, ldg_u=d_, act=1 if d_ % 2 else 3, pad_fill=0.3)
for mode_, inner_ in ((0, True), (0, False), (1, False)):              # both modes, inner residual on / off, every act code
    for act_ in (0, 1, 2, 3, 4):
        _add('act', f'mode{mode_}_inner{int(inner_)}_act{act_}', T=32, d=16, mode=mode_, inner=inner_, act=act_)
for T_ in (32, 17):                                                    # > 2 workgroups per CU on 256 CUs: the launch wraps
    _add('big', f'big_T{T_}', B=600, T=T_, d=16)
for T_ in (17, 32):                                                    # dropout with the kernel's own masks
    for mode_ in (0, 1):
        for tag, pa, ph in (('both', 0.1, 0.1), ('attn', 0.1, 0.0), ('hidden', 0.0, 0.1)):
            _add('drop', f'drop_T{T_}_mode{mode_}_{tag}', T=T_, d=16, mode=mode_, inner=mode_ == 0, drop_attn=pa, drop_hidden=ph,
                 drop_seed=0x5eed * 1000003 + 7)


def names(group):
    return [n for n, s in CASES.items() if s['group'] == group]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case and its fp64 reference, computed once per process and shared (read-only) by every test that needs it.  For a many-user
    case dy is zeroed for the users near a kink BEFORE the backward reference runs; `kink` says which."""
    spec = {k: v for k, v in CASES[name].items() if k != 'group'}
    desc, x, mask, dy = make_case(**spec)
    B, T = spec['B'], spec['T']
    masks = None
    if spec.get('drop_attn', 0.0) or spec.get('drop_hidden', 0.0):
        masks = dropout_multipliers(desc['drop_seed'], desc['drop_site'], B, T, desc['drop_attn'], desc['drop_hidden'])
    kink = near_kink_users(block_ref(desc, x, mask, T, masks=masks).pre)
    if B > 8:
        dy.view(B, T, E)[kink] = 0
    ref = block_ref(desc, x, mask, T, dy=dy, masks=masks)
    return SimpleNamespace(name=name, spec=CASES[name], desc=desc, x=x, mask=mask, dy=dy, masks=masks, ref=ref, kink=kink, B=B, T=T, d=spec['d'])
