"""The parameter-side kernels -- a4r_lora_bwd_fused (csrc/a4r_lora.hip), a4r_lora_merge, a4r_lora_merge_batch, a4r_phm_build, a4r_phm_bwd,
a4r_unpack_add (csrc/a4r_params.hip), a4r_pack_matrices (csrc/a4r_head.hip) -- against the fp64 references of tests/param_ref.py at their shape
and launch edges, on the cases tests/test_param_ref_cpu.py proves sound.  param_ref's header states the formulas, the buffers (strided views with
junk in the gaps, sentinels or non-zero bases in every output), the bounds and which case runs which branch.  References are computed on the
device in fp64, once per case.

G = a4r_lora_bwd_fused_ws_floats(768) // (64 * 768): the workgroups of the LoRA kernel, one per CU.  The integer LoRA cases must equal the fp64
reference BIT FOR BIT at 1, 2, 3, 5, G-1, G, G+1, 2G, 2G+1 and 3G+1 tiles in all four rank forms: one lost, doubled or misplaced tile fails.

REJECTIONS.  Every argument check of the seven entry points has a call that trips it; the entry returns A4R_EINVAL before anything is launched
(only values that are refused ahead of the launch are used), and every output keeps its sentinels and bases.  The unmodified call of each
template returns A4R_OK, so that a refusal is the refusal of the one argument changed.

MEASURED on an MI355X (G = 256; the KERNEL lines the tests print: per output buffer the worst error over its bound and, in brackets, the largest
error).  102 tests in 2.6 s; the slowest, the first launch of the process aside (1.2 s), 0.16 s (merge_bf16_768x768_r1), every LoRA case 0.01 s
but the first random one (0.08 s).
    a4r_lora_bwd_fused   40 integer cases: every buffer exact.  8 random cases: dA 0.54 of its bound (5.9e-03: lora_rand0_tG+1_8_1_8), dB_q / dB_v and
                         their bias column 0.56 (2.9e-03 / 1.2e-03: lora_rand1_tG+1_16_12_12), the contiguous bias sums 0.01 (1.7e-06).  Errors of that
                         size are one-ulp flips of t / dt at near ties, which the allowance is for: near-tie pairs are 0.90 % .. 0.92 % of the
                         live (row, rank) pairs.
    a4r_lora_merge       bf16 0.25 of the bound in every case (7.7e-03 .. 3.1e-02: the model's own rounding), fp32 at most 0.26 (4.0e-07:
                         merge_f32_192x192_r12); a4r_lora_merge_batch: 0.25 in both types, the r = 0 projection exact in fp32; dst and dstT
                         bit-equal at transposed positions everywhere.
    a4r_phm_build        at most 0.25 of the fp32 bound (2.2e-08).  a4r_phm_bwd: at most 0.01 of C_PHM = 64 units, i.e. under one unit of
                         2^-24 (|base| + sum |term|) (1.8e-06: phm_trio) -- a wave sums its lanes pairwise, far from the sequential fp32
                         restatement that set the constant.
    a4r_unpack_add       at most 0.21 of the fp32 bound (2.1e-07: unpack_offset2).
    a4r_pack_matrices    all 24 destinations exact through both kernels in both output types, the two kernels bit-equal.

Hand mutations of a scratch copy of the three .hip files (never committed; every one in bounds, wrong results only), built into a second library
and run through this file: 47 of the 102 tests fail, each mutation exactly where its branch runs.  The narrow LoRA kernel's next-tile request always
re-requesting the tile itself: every narrow case beyond G tiles (G+1, 2G, 2G+1, 3G+1, the random ones), none at G tiles or fewer.  The reduction's
tail loop one slice short, wide form only: the wide cases at 1, 2, 3, 5 and G-1 tiles, none from G tiles on (chunks of 64).  a4r_lora_merge without
its grid stride: the ten 768 x 768 cases alone.  store4's element fallback writing 3 of 4: mbatch_* at the two offset slots (d3 / t3, d4 / t4).
a4r_unpack_add without its stride: unpack_true, _small, _offset2, not _offset0 (16 elements).  rule[k][b][a] in d Wl of phm_bwd: every PHM case
but n = 1.  The tiled pack kernel without its stride: p2 / p3 (320 x 320: 25 tiles on 16 workgroups) of pack_*_tiled alone.
"""
import functools

import pytest
import torch

import param_ref as P
from attn_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL = -1
SPECS = P.specs(P.G_NOMINAL)                                  # (the names do not depend on G; the row counts of the G-labelled LoRA cases do)


def names(family, part=''):
    return [s['name'] for s in SPECS[family] if part in s['name']]


@functools.lru_cache(maxsize=None)
def lib():
    from adapter4rec_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def G():
    return lib().lib().a4r_lora_bwd_fused_ws_floats(P.H) // (64 * P.H)


@functools.lru_cache(maxsize=None)
def table():
    return {s['name']: (fam, s) for fam, ss in P.specs(G()).items() for s in ss}


def check(name):
    fam, spec = table()[name]
    c = P.build(fam, spec, DEV)
    got = P.run(c, lib())
    figures, fails = P.judge(c, got)
    print('KERNEL ' + P.table_row(c, figures))
    assert set(figures) == set(c.expect) and not fails, (name, fails)
    return c, got


@pytest.mark.parametrize('name', names('lora', '_int_'))
def test_lora_bwd_fused_integer_cases_are_bit_exact(name):
    """exact small-integer operands: every fp32 partial sum is exact in any order, so the kernel equals the fp64 reference bit for bit -- the
    grid-stride loop, the one-tile-ahead request and the four-chunk reduction of the workgroups' slices can neither drop nor double a tile"""
    c, _ = check(name)
    exact, mag = P.lora_exactness(c)
    assert c.tiles == P.tiles_of(name.split('_t')[1].split('_')[0], G()) and exact and mag < 2.0 ** 22, (c.tiles, exact, mag)
    assert all(float(b.max()) == 0 for _, b in c.expect.values())


@pytest.mark.parametrize('name', names('lora', '_rand'))
def test_lora_bwd_fused_random_cases(name):
    """the rounding model at G + 1 tiles: t and dt rounded to bf16 from fp32 sums, fp32 accumulation across tiles and workgroups"""
    c, _ = check(name)
    print(f'NEAR {name}: {c.near_share:.4%} of the live (row, rank) pairs')
    assert c.near_share <= 0.02


@pytest.mark.parametrize('name', names('merge'))
def test_lora_merge(name):
    check(name)


@pytest.mark.parametrize('name', names('phm'))
def test_phm_build_and_bwd(name):
    check(name)


@pytest.mark.parametrize('name', names('unpack'))
def test_unpack_add(name):
    check(name)


@pytest.mark.parametrize('dt', P.DTYPES)
def test_pack_matrices_both_kernels(dt):
    """the tiled and the element-wise kernel on the same descriptors: both equal the one-rounding cast of the source, hence each other, bit for bit"""
    (_, tiled), (_, elem) = check(f'pack_{dt}_tiled'), check(f'pack_{dt}_elem')
    assert set(tiled) == set(elem) and all(torch.equal(tiled[k], elem[k]) for k in tiled)


# ------------------------------------------------------------------ argument refusals
def _ptr(t):
    return t.data_ptr()


@functools.lru_cache(maxsize=None)
def _templates():
    """entry point -> (ordered arguments of a valid call, the output tensors that must stay as they are when the call is refused)"""
    L = lib()
    H = P.H
    t = {}
    c = P.make_lora('reject', 1, 8, 8, 5, 'int', 'col', DEV)
    i, o = c.inputs, P.lora_outputs(c)
    ws = torch.full((G() * 64 * H,), SENTINEL, device=DEV)
    t['a4r_lora_bwd_fused'] = (dict(
        x=_ptr(i['x']), ldx=H + 8, dqa=_ptr(i['dqkv']), dqb=_ptr(i['dqkv'][:, 2 * H:]), lddq=3 * H, Aa=_ptr(i['A']), Ab=_ptr(i['A'][16:]), BTa=_ptr(i['BTa']),
        BTb=_ptr(i['BTb'][16:]), ldw=H, sa=0.5, sb=2.0, dAa=_ptr(o['sA']), dAb=_ptr(o['sA'][16:]), lda=H, dBa=_ptr(o['sBq']), dBb=_ptr(o['sBv'][:, 16:]), ldb=P.RP,
        dba=_ptr(o['sBq'][:, P.OC:]), dbb=_ptr(o['sBv'][:, P.OC:]), ldbias=P.RP, M=16, H=H, dtype=L.BF16, rank_rows=8, ws=_ptr(ws), ws_floats=ws.numel()),
        list(o.values()) + [ws], c)
    W, Am, Bm = torch.randn(72, 40, device=DEV), torch.randn(4, 40, device=DEV), torch.randn(72, 4, device=DEV)
    d, dT = torch.full((72, 48), SENTINEL, device=DEV), torch.full((40, 80), SENTINEL, device=DEV)
    t['a4r_lora_merge'] = (dict(W=_ptr(W), A=_ptr(Am), B=_ptr(Bm), s=0.5, dst=_ptr(d), ld=48, dstT=_ptr(dT), ldT=80, out_f=72, in_f=40, r=4, dtype=L.F32), [d, dT],
                           (W, Am, Bm))
    tab, n, mx, code = L.lora_table([(W, Am, Bm, 0.5, d[:, :40], dT[:, :72], 4)], DEV)
    t['a4r_lora_merge_batch'] = (dict(desc=_ptr(tab), n_desc=n, max_elems=mx, dtype=code), [d, dT], tab)
    pc = P.make_phm('reject', [(2, 8, 8, 0, 0)], DEV)
    ptab = L.desc_table(pc.descs, DEV)
    eff, grads = torch.full((pc.eff_len,), SENTINEL, device=DEV), pc.base.clone()
    t['a4r_phm_build'] = (dict(params=_ptr(pc.inputs['params']), desc=_ptr(ptab), n_desc=1, eff=_ptr(eff)), [eff], (pc, ptab))
    t['a4r_phm_bwd'] = (dict(params=_ptr(pc.inputs['params']), desc=_ptr(ptab), n_desc=1, grads=_ptr(grads)), [grads], (pc, ptab))
    uc = P.make_unpack('reject', 'true', DEV)
    utab, target = L.desc_table(uc.descs, DEV), uc.base.clone()
    t['a4r_unpack_add'] = (dict(target=_ptr(target), desc=_ptr(utab), n_desc=len(uc.descs), max_elems=uc.max_elems), [target], (uc, utab))
    flat, pd = torch.randn(16 * 64, device=DEV), torch.full((64, 64), SENTINEL, device=DEV)
    ktab = L.desc_table([L.PackDesc(0, _ptr(pd), 16, 64, 64, 64, 0, 0)], DEV)
    t['a4r_pack_matrices'] = (dict(flat=_ptr(flat), desc=_ptr(ktab), n_desc=1, max_elems=4096, dtype=L.F32), [pd], (flat, ktab))
    torch.cuda.synchronize()
    return t


FP8 = 2                       # A4R_FP8: a dtype code none of these entry points takes
REJECTIONS = {
    'a4r_lora_bwd_fused': [dict(x=None), dict(dqa=None), dict(dqb=None), dict(Aa=None), dict(Ab=None), dict(BTa=None), dict(BTb=None), dict(dAa=None),
                           dict(dAb=None), dict(dBa=None), dict(dBb=None), dict(ws=None), dict(M=0), dict(M=24), dict(M=-16), dict(H=384), dict(dtype=1),
                           dict(rank_rows=12), dict(ldb=7), dict(rank_rows=16, ldb=14), dict(ldx=760), dict(lddq=760), dict(ldw=760), dict(lda=760),
                           dict(ldx=772), dict(lddq=2308), dict(ldw=772), dict(x='+2'), dict(dqb='+2'), dict(BTa='+2'), dict(ldbias=0), dict(dba=None, ldbias=0),
                           dict(ws_floats=34 * 768 - 1), dict(rank_rows=16, ws_floats=64 * 768 - 1)],
    'a4r_lora_merge': [dict(W=None), dict(dst=None), dict(dstT=None), dict(out_f=0), dict(in_f=0), dict(r=-1), dict(A=None), dict(B=None), dict(ld=39), dict(ldT=71),
                       dict(dtype=FP8), dict(dtype=7)],
    'a4r_lora_merge_batch': [dict(desc=None), dict(n_desc=0), dict(max_elems=0), dict(dtype=FP8)],
    'a4r_phm_build': [dict(params=None), dict(desc=None), dict(n_desc=0), dict(eff=None)],
    'a4r_phm_bwd': [dict(params=None), dict(desc=None), dict(n_desc=0), dict(grads=None)],
    'a4r_unpack_add': [dict(target=None), dict(desc=None), dict(n_desc=0), dict(max_elems=0)],
    'a4r_pack_matrices': [dict(flat=None), dict(desc=None), dict(n_desc=0), dict(max_elems=0), dict(dtype=FP8)],
}


@pytest.mark.parametrize('entry', list(REJECTIONS))
def test_argument_checks_refuse_before_launch(entry):
    L = lib()
    assert L.FP8 == FP8 and L.F32 == 1
    args, outs, _keep = _templates()[entry]
    fn = getattr(L.lib(), entry)
    call = lambda a: fn(torch.cuda.current_stream().cuda_stream, *a.values())
    before = [o.clone() for o in outs]
    for change in REJECTIONS[entry]:
        a = dict(args)
        for k, v in change.items():
            assert k in a, k
            a[k] = a[k] + 2 if v == '+2' else v
        rc = call(a)
        torch.cuda.synchronize()
        assert rc == EINVAL, (entry, change, rc)
        assert all(torch.equal(b, o) for b, o in zip(before, outs)), (entry, change, 'an output was written')
    assert call(dict(args)) == 0, (entry, 'the template itself is refused')
    torch.cuda.synchronize()
