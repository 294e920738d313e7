"""fp64 references of the parameter-side kernels -- the ones that produce the only trainable gradients and the only trained weights of a LoRA or
Compacter run -- and the cases their tests share: a4r_lora_bwd_fused (csrc/a4r_lora.hip), a4r_lora_merge, a4r_lora_merge_batch, a4r_phm_build,
a4r_phm_bwd, a4r_unpack_add (csrc/a4r_params.hip), a4r_pack_matrices (csrc/a4r_head.hip).  TEST INFRASTRUCTURE ONLY.
tests/test_param_ref_cpu.py proves this file sound on the CPU (independent formulations, the fp32 restatement of tests/sim_lib.py, mutation
checks, the constants, branch coverage); tests/test_param_kernels_gpu.py runs the kernels through it.  The formulas are those of include/a4r.h and
of the comments at the top of the two .hip files:

    LoRA backward   t = bf16(x [A_q ; A_v]^T) ; dt = bf16((dq B_q) s_q | (dv B_v) s_v) ; dA_q | dA_v += dt^T x ; dB_q += dq^T t_q ; dB_v += dv^T t_v
                    (unscaled) ; db_q += column sums of dq, db_v of dv.  rank_rows 8: dA [8, H] and dB [H, 8] per LoRA; 16: [16, H] and [H, 15].
                    Rank rows past a LoRA's r are zero, so their gradients are exact zeros added to the base.
    LoRA merge      dst[o, i] = dstT[i, o] = W[o, i] + s sum_k B[o, k] A[k, i], rounded once to the output type.
    PHM             E[b oq + q][a ip + p] = sum_k rule[k][a][b] Wl[k][p] Wr[k][q], ip = in / n, oq = out / n; with G = dL/dE [out, in] at row
                    stride ldg: d rule[k][a][b] += sum_{q,p} G Wl Wr ; d Wl[k][p] += sum_{a,b,q} G rule Wr ; d Wr[k][q] += sum_{a,b,p} G rule Wl.
    unpack_add      target[dst_off + r cols + c] += alpha src[r ld + c].
    pack            dst[rows_pad, cols_pad] = src [rows, cols] or its transpose, zero padded, rounded once; layout 0 row-major at dst_ld (0: cols_pad);
                    layouts 1 / 2: MFMA fragment order (frag_map: written from the fragment description, as the inverse map index -> (row, column)).

BUFFERS.  Every strided operand is a view into a wider buffer; gap columns, the rows at or beyond M and the unused rank rows of the 64-row weight
operands hold JUNK; contiguous inputs are followed by JUNK.  Every output buffer is pre-filled with SENTINEL or a non-zero base (all these kernels
accumulate or write slots).  A case carries, per output buffer, the WHOLE expected buffer and a bound of the same shape that is 0 wherever the
buffer must hold exactly what is expected: the surroundings of every slot, and every element of an exact case.  run_* also checks that no input
changed.  LoRA operands are laid out as the engine lays them: dq / dv are columns 0 .. H and 2 H .. 3 H of a fused [M, 3 H] gradient, the weights
rank rows 0 .. and 16 .. of 64-row operands, dA rows 0 .. / 16 .. of a [64, H] fp32 scratch, dB columns 0 .. / 16 .. of [H, 64] scratches, the bias
sums column 32 of those (ldbias = 64) or contiguous vectors between sentinels (ldbias = 1).

BOUNDS -- the project's rules (tests/adapter_ln_ref.py, tests/ln_rows_ref.py), not new numbers:
  * exact-integer LoRA cases and every pack case: equality.  Integer operands: x, dq, dv in {-2 .. 2}, every live weight rank row 32 entries of
    +-1 at random columns, s_q = 0.5, s_v = 2: t and dt are exact in bf16 and every sum of |term| stays below 2^22 (lora_exactness; the outputs sit
    on bases of 0.5 and +-0.25, two bits below the integers, hence 2^22 and not 2^24), so every fp32 partial sum is exact in any order and ONE
    lost, doubled or misplaced tile changes bits.
  * fp32 outputs (fp32 merge, phm_build, unpack_add) against fp64: four times the largest error over the tensor of the same formula evaluated
    in fp32 on the CPU (torch's own reductions), floor 2^-22 of the tensor's magnitude.
  * bf16 merge: every element within twice the model's largest error (the fp64 value rounded once) plus one bf16 ulp of the reference; dst
    and dstT hold the same bits at transposed positions (both types).
  * sums flushed by atomics (phm_bwd, the random LoRA cases): |got - (base + ref)| <= C 2^-24 (|base| + sum |term|), the terms from the
    reference, C = adapter_ln_ref.C_SUM = 16 for the LoRA sums.  PHM terms are products of three fp32 factors: tests/test_param_ref_cpu.py evaluates
    these sums in fp32, term by term (both products rounded), in a shuffled order onto the base: 4 x the worst ratio is 38.3, NOT <= C_SUM, so
    phm_bwd is held to the family constant C_PHM = 64 (4 x the worst CPU ratio rounded up to a power of two; both numbers at C_PHM below).
  * random LoRA cases, in addition: t and dt are rounded to bf16 from fp32 sums in an order the reference does not share.  A (row, rank) whose
    fp64 value lies within 2^-22 sum_k |x A| of a bf16 rounding boundary may flip by one bf16 ulp: sum over those near-tie rows of
    |operand[row, col]| ulp_bf16(t[row, rank]) is added to that element's bound.  near-tie pairs are at most 2 % of the live (row, rank) pairs
    (asserted on the CPU; lora cases carry the share as c.near_share).

CASES and the BRANCH each one runs (branches(); G = the LoRA kernel's workgroup count = a4r_lora_bwd_fused_ws_floats(768) // (64 * 768), 256
on an MI355X; the CPU file builds the same tables at G = 8 and checks the coverage at both):
    lora_*_t<tiles>_<R>_<rq>_<rv>   tiles 1, 2, 3, 5, G-1, G, G+1, 2G, 2G+1, 3G+1 x (R, r_q, r_v) (8,8,5) (8,1,8) (16,12,12) (16,15,9), integer;
                                    rand at G+1, two seeds per form.  narrow / wide: lora_bwd_kernel / lora_bwd2_kernel.  tiles <= G: one tile per
                                    workgroup, the prefetch re-requests the tile itself ('self_prefetch'); G+1, 2G+1, 3G+1: workgroup 0 runs one
                                    tile more than the others ('ragged_round'); 2G: 'full_rounds'.  The reduction sums nblk = min(tiles, G) slices in
                                    4 chunks of ceil(nblk / 4): 'chunk_empty' (tiles 1, 2, 3, 5), 'chunk_tail_only' (fewer than 4 slices: tiles 1 .. 5),
                                    'chunk_unrolled' (a multiple of 4: G), 'chunk_unrolled_tail' (G-1: 64, 64, 64, 63).  Bias sinks: both in column 32
                                    ('col'), both contiguous ('vec'), q alone in the column, v alone contiguous, none.
    merge_<dt>_<out>x<in>_r<r>      a4r_lora_merge: 768 x 768 ('single_stride': beyond 1024 x 256 elements), 192 x 192, 72 x 40 ('single_pass');
                                    r 0, 1, 8, 12, 16.
    mbatch_<dt>                     a4r_lora_merge_batch, one table: 768 x 768 r 8 and 64 x 64 r 4 ('batch_tiled', 'store4_vector'), 320 x 264 r 12
                                    ('batch_elem_stride': 84 480 elements > 65 536), 128 x 64 r 8 with slots 2 resp. 1 elements into a row
                                    ('store4_fallback'), 64 x 128 r 0 with null A / B ('batch_r0').
    phm_*                           (n, in, out) (1,64,16) (2,8,8) (4,8,8: oq ip = 4 < 64, 'short_reduction') (4,768,48: 64 scratch rows, 'out_padded')
                                    (4,48,768: ldg 64, 'ldg_padded') (8,768,64) (16,64,768: ldg 72); phm_pair 768 -> 64 -> 768 and phm_trio (+ 768 -> 48)
                                    on one rule ('shared_rule'); grads start from a non-zero base.  Everything of a gradient scratch outside its
                                    [out, in] block holds JUNK, not the engine's zeros: a kernel that read its padding would show.
    unpack_<mode>                   descriptors 1 x 16, 16 x 80, 130 x 130 (ld 136), 300 x 64; alpha 1, 0.5, -0.25, 1; 'true' max_elems (19 200: the
                                    grid cap of 16 384 makes 130 x 130 and 300 x 64 stride: 'unpack_stride'), 'small' max_elems 1280 (every larger
                                    descriptor strides), 'offset' (one descriptor at tab[j bytes:]: 'table_offset').
    pack_<dt>_<kernel>              'tiled' (max_elems 65 536: 16 workgroups in x) and 'elem' (the true max_elems, capped at 65 535 so that the
                                    dispatch stays element-wise; 320 x 320 then strides): destinations 16x64 -> 64x64, 300x257 -> 320x320 at dst_ld 960
                                    (25 tiles > 16: 'tiled_stride'), 70x130 -> 128x192, 1x1 -> 64x64, each plain and transposed; layouts 1 and 2 at
                                    H 128, 256, 768, 1024, plain and transposed.
"""
import ctypes
import functools
from types import SimpleNamespace

import torch

import adapter_ln_ref as A
from attn_ref import JUNK, SENTINEL, rb

C_SUM = A.C_SUM
# The PHM sums by adapter_ln_ref's rule (fp32, term by term, both products rounded, shuffled, one after the other onto the base;
# tests/test_param_ref_cpu.py::test_c_sum_does_not_cover_the_phm_sums_and_c_phm_does): worst ratio 9.57 (d rule of phm_n16_64_768: 4096 sums of 192
# terms on bases up to 4 that outweigh them), 6.16 for d Wl (phm_n8_768_64), 6.16 for d Wr (phm_n4_48_768) -> 4 x 9.57 = 38.3 > C_SUM = 16: the PHM
# family gets its own constant, 38.3 rounded up to a power of two.  From the fp32 restatement, never from the kernel.
C_PHM = 64.0
H = 768
G_NOMINAL = 256
F32, BF16 = torch.float32, torch.bfloat16
DT = {'f32': F32, 'bf16': BF16}
DTYPES = ('bf16', 'f32')


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _tail(n, device, fill=JUNK, dtype=F32, extra=16):
    """a contiguous [n] tensor (16-byte aligned) followed by `extra` elements of fill"""
    buf = torch.full((n + extra,), fill, dtype=dtype, device=device)
    return buf, buf[:n]


def _round(v, T):
    """fp64 values as a tensor of type T stores them, back in fp64"""
    return rb(v) if T == BF16 else v.float().double()


def seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def judge(c, got):
    """got: name -> the whole output buffer.  Returns (figures, failures); figures[name] = (largest error, worst error / bound where a bound is
    given, elements that had to be exact and are not)."""
    figures, fails = {}, []
    for k, (want, bound) in c.expect.items():
        if k not in got:
            fails.append(f'{k}: missing')
            continue
        g = got[k].double()
        if g.shape != want.shape:
            fails.append(f'{k}: shape {tuple(g.shape)}, wanted {tuple(want.shape)}')
            continue
        if not bool(torch.isfinite(g).all()):
            fails.append(f'{k}: non-finite')
            continue
        err = (g - want).abs()
        live = bound > 0
        ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
        wrong = int(((err > 0) & ~live).sum())
        if wrong:
            i = int(((err > 0) & ~live).view(-1).nonzero()[0])
            fails.append(f'{k}: {wrong} elements that must be exact are not; the first at flat index {i}: {float(g.view(-1)[i])!r}, wanted {float(want.view(-1)[i])!r}')
        if ratio > 1:
            i = int(torch.where(live, err / bound.clamp(min=1e-300), torch.zeros_like(err)).view(-1).argmax())
            fails.append(f'{k}: flat index {i} off by {float(err.view(-1)[i]):.3e}, {ratio:.3g} x its bound {float(bound.view(-1)[i]):.3e}')
        figures[k] = (float(err.max()), ratio, wrong)
    for a, b in getattr(c, 'same_bits', ()):
        if a in got and b in got and not torch.equal(c.slot[a](got[a]), c.slot[b](got[b]).t()):
            fails.append(f'{a} and {b} differ at transposed positions')
    return figures, fails


def _unchanged(c, before):
    for k, b in before.items():
        assert torch.equal(b, c.inputs[k]), f'{c.name}: input {k} was written'


def _sync(c):
    if c.device != 'cpu':
        torch.cuda.synchronize()


def table_row(c, figures):
    return f'{c.name:<34}|' + ''.join(f' {k} {f[1]:.2f} ({f[0]:.1e})' if f[1] > 0 or f[0] > 0 else f' {k} exact' for k, f in figures.items())


# ================================================================== a4r_lora_bwd_fused
LORA_FORMS = ((8, 8, 5), (8, 1, 8), (16, 12, 12), (16, 15, 9))
TILE_LABELS = ('1', '2', '3', '5', 'G-1', 'G', 'G+1', '2G', '2G+1', '3G+1')
BIAS_MODES = ('col', 'vec', 'q_col', 'v_vec', 'none')
RP, OC = 64, 32                      # rows of the padded rank dimension; the column the bias sums share with the engine's ones column
BASE_A, BASE_BQ, BASE_BV, BASE_VEC = 0.5, 0.25, -0.25, 0.125


def tiles_of(label, G):
    return {'1': 1, '2': 2, '3': 3, '5': 5, 'G-1': G - 1, 'G': G, 'G+1': G + 1, '2G': 2 * G, '2G+1': 2 * G + 1, '3G+1': 3 * G + 1}[label]


def lora_specs(G):
    specs = []
    for i, lab in enumerate(TILE_LABELS):
        for j, (R, rq, rv) in enumerate(LORA_FORMS):
            specs.append(dict(name=f'lora_int_t{lab}_{R}_{rq}_{rv}', tiles=tiles_of(lab, G), R=R, rq=rq, rv=rv, kind='int', bias=BIAS_MODES[(i + j) % 5]))
    for j, (R, rq, rv) in enumerate(LORA_FORMS):
        for s in (0, 1):
            specs.append(dict(name=f'lora_rand{s}_tG+1_{R}_{rq}_{rv}', tiles=G + 1, R=R, rq=rq, rv=rv, kind='rand', bias=BIAS_MODES[(2 * j + s) % 5]))
    return specs


def lora_branches(tiles, R, bias, G):
    out = {'narrow' if R == 8 else 'wide', 'bias_' + bias}
    out.add('single_tile' if tiles == 1 else 'self_prefetch' if tiles <= G else 'full_rounds' if tiles % G == 0 else 'ragged_round')
    nblk = min(tiles, G)
    per = (nblk + 3) // 4
    for y in range(4):
        n = max(0, min(per, nblk - y * per))
        out.add('chunk_empty' if n == 0 else 'chunk_tail_only' if n < 4 else 'chunk_unrolled' if n % 4 == 0 else 'chunk_unrolled_tail')
    return out


def make_lora(name, tiles, R, rq, rv, kind, bias, device='cpu', seed=None):
    g = _gen(device, seed_of(name) if seed is None else seed)
    M, nb = 16 * tiles, R - (R == 16)
    Mb = M + 16
    if kind == 'int':
        ri = lambda *s: torch.randint(-2, 3, s, generator=g, device=device).to(BF16)
        x, dq, dv = ri(M, H), ri(M, H), ri(M, H)

        def w(r):
            W = torch.zeros(R, H, device=device)
            cols = torch.rand(R, H, generator=g, device=device).argsort(1)[:, :32]
            W.scatter_(1, cols, (torch.randint(0, 2, (R, 32), generator=g, device=device) * 2 - 1).float())
            W[r:] = 0
            return W.to(BF16)
        sq, sv = 0.5, 2.0
    else:
        rn = lambda *s: torch.randn(*s, generator=g, device=device)
        x, dq, dv = rn(M, H).to(BF16), (rn(M, H) * 0.1).to(BF16), (rn(M, H) * 0.1).to(BF16)

        def w(r):
            W = rn(R, H) * 0.05
            W[r:] = 0
            return W.to(BF16)
        sq, sv = 0.125, 2.0
    Aq, Av, Bq, Bv = w(rq), w(rv), w(rq), w(rv)                     # Bq, Bv: B^T, [rank rows, H]
    xbuf = torch.full((Mb, H + 8), JUNK, dtype=BF16, device=device)
    xbuf[:M, :H] = x
    gbuf = torch.full((Mb, 3 * H), JUNK, dtype=BF16, device=device)
    gbuf[:M, :H], gbuf[:M, 2 * H:] = dq, dv
    Ab, BTa, BTb = (torch.full((RP, H), JUNK, dtype=BF16, device=device) for _ in range(3))
    Ab[0:R], Ab[16:16 + R], BTa[0:R], BTb[16:16 + R] = Aq, Av, Bq, Bv
    c = SimpleNamespace(name=name, family='lora', tiles=tiles, M=M, R=R, rq=rq, rv=rv, nb=nb, kind=kind, bias=bias, sq=sq, sv=sv, device=device,
                        inputs=dict(x=xbuf, dqkv=gbuf, A=Ab, BTa=BTa, BTb=BTb))
    X, Q, V = x.double(), dq.double(), dv.double()
    aq, av, bq, bv = Aq.double(), Av.double(), Bq.double(), Bv.double()
    raw = dict(tq=X @ aq.t(), tv=X @ av.t(), dtq=(Q @ bq.t()) * sq, dtv=(V @ bv.t()) * sv)
    t = {k: rb(v) for k, v in raw.items()}
    ref = dict(dAq=t['dtq'].t() @ X, dAv=t['dtv'].t() @ X, dBq=(Q.t() @ t['tq'])[:, :nb], dBv=(V.t() @ t['tv'])[:, :nb], dbq=Q.sum(0), dbv=V.sum(0))
    ab = dict(dAq=t['dtq'].abs().t() @ X.abs(), dAv=t['dtv'].abs().t() @ X.abs(), dBq=(Q.abs().t() @ t['tq'].abs())[:, :nb],
              dBv=(V.abs().t() @ t['tv'].abs())[:, :nb], dbq=Q.abs().sum(0), dbv=V.abs().sum(0))
    c.ref, c.abs, c.t_raw, c.t = ref, ab, raw, t
    # near ties of the bf16 rounding of t and dt, and what a flip of one ulp moves
    slack = dict(tq=X.abs() @ aq.abs().t(), tv=X.abs() @ av.abs().t(), dtq=(Q.abs() @ bq.abs().t()) * sq, dtv=(V.abs() @ bv.abs().t()) * sv)
    flip, near_n, live_n = {}, 0, 0
    for k, u in raw.items():
        ulp = A.ulp_bf16(u)
        near = (ulp / 2 - (u - t[k]).abs()) <= 2.0 ** -22 * slack[k]
        near &= slack[k] > 0
        flip[k] = near * A.ulp_bf16(t[k]).clamp(min=ulp)
        r = rq if k.endswith('q') else rv
        near_n, live_n = near_n + int(near[:, :r].sum()), live_n + M * r
    c.near_share = near_n / live_n
    extra = dict(dAq=flip['dtq'].t() @ X.abs(), dAv=flip['dtv'].t() @ X.abs(), dBq=(Q.abs().t() @ flip['tq'])[:, :nb], dBv=(V.abs().t() @ flip['tv'])[:, :nb],
                 dbq=torch.zeros(H, dtype=torch.float64, device=device), dbv=torch.zeros(H, dtype=torch.float64, device=device))

    def bnd(k, base):
        if kind == 'int':
            return torch.zeros_like(ref[k])
        return C_SUM * 2.0 ** -24 * (abs(base) + ab[k]) + extra[k]
    f64 = lambda *s, v: torch.full(s, v, dtype=torch.float64, device=device)
    eA, bA = f64(RP, H, v=BASE_A), f64(RP, H, v=0.0)
    eBq, bBq, eBv, bBv = f64(H, RP, v=BASE_BQ), f64(H, RP, v=0.0), f64(H, RP, v=BASE_BV), f64(H, RP, v=0.0)
    eV, bV = f64(2 * (H + 8) + 8, v=SENTINEL), f64(2 * (H + 8) + 8, v=0.0)
    eA[0:R] += ref['dAq']
    eA[16:16 + R] += ref['dAv']
    bA[0:R], bA[16:16 + R] = bnd('dAq', BASE_A), bnd('dAv', BASE_A)
    eBq[:, 0:nb] += ref['dBq']
    eBv[:, 16:16 + nb] += ref['dBv']
    bBq[:, 0:nb], bBv[:, 16:16 + nb] = bnd('dBq', BASE_BQ), bnd('dBv', BASE_BV)
    c.vec_at = (8, H + 16)
    for at in c.vec_at:
        eV[at:at + H] = BASE_VEC
    if bias in ('col', 'q_col'):
        eBq[:, OC] += ref['dbq']
        bBq[:, OC] = bnd('dbq', BASE_BQ)
    if bias == 'col':
        eBv[:, OC] += ref['dbv']
        bBv[:, OC] = bnd('dbv', BASE_BV)
    if bias == 'vec':
        eV[8:8 + H] += ref['dbq']
        bV[8:8 + H] = bnd('dbq', BASE_VEC)
    if bias in ('vec', 'v_vec'):
        eV[H + 16:2 * H + 16] += ref['dbv']
        bV[H + 16:2 * H + 16] = bnd('dbv', BASE_VEC)
    c.expect = dict(sA=(eA, bA), sBq=(eBq, bBq), sBv=(eBv, bBv), vec=(eV, bV))
    return c


def lora_exactness(c):
    """(t and dt are exact in bf16, the largest |base| + sum |term| of any output)"""
    exact = all(torch.equal(c.t[k], c.t_raw[k]) for k in c.t)
    return exact, max(float(v.max()) for v in c.abs.values()) + 0.5


def lora_outputs(c):
    dev = c.device
    sA = torch.full((RP, H), BASE_A, device=dev)
    sBq, sBv = torch.full((H, RP), BASE_BQ, device=dev), torch.full((H, RP), BASE_BV, device=dev)
    vec = torch.full((2 * (H + 8) + 8,), SENTINEL, device=dev)
    for at in c.vec_at:
        vec[at:at + H] = BASE_VEC
    return dict(sA=sA, sBq=sBq, sBv=sBv, vec=vec)


def lora_bias_views(c, o):
    va, vb = o['vec'][c.vec_at[0]:c.vec_at[0] + H], o['vec'][c.vec_at[1]:c.vec_at[1] + H]
    return {'col': (o['sBq'][:, OC], o['sBv'][:, OC]), 'vec': (va, vb), 'q_col': (o['sBq'][:, OC], None), 'v_vec': (None, vb), 'none': (None, None)}[c.bias]


def run_lora(c, L):
    before = {k: b.clone() for k, b in c.inputs.items()}
    o = lora_outputs(c)
    i, R = c.inputs, c.R
    ba, bb = lora_bias_views(c, o)
    L.lora_bwd_fused(i['x'][:, :H], i['dqkv'][:, :H], i['dqkv'][:, 2 * H:], i['A'][0:R], i['A'][16:16 + R], i['BTa'][0:R], i['BTb'][16:16 + R], c.sq, c.sv,
                     o['sA'][0:R], o['sA'][16:16 + R], o['sBq'][:, 0:R], o['sBv'][:, 16:16 + R], ba, bb, c.M, rank_rows=R)
    _sync(c)
    _unchanged(c, before)
    return o


# ================================================================== a4r_lora_merge / a4r_lora_merge_batch
MERGE_SHAPES = ((768, 768), (192, 192), (72, 40))
MERGE_RANKS = (0, 1, 8, 12, 16)
# (out, in, r, elements into a row at which the dst / dstT slots start: bf16, fp32)
BATCH_TABLE = ((768, 768, 8, (0, 0)), (64, 64, 4, (0, 0)), (320, 264, 12, (0, 0)), (128, 64, 8, (2, 1)), (128, 64, 8, (2, 2)), (64, 128, 0, (0, 0)))


def merge_specs():
    specs = [dict(name=f'merge_{dt}_{o}x{i}_r{r}', dt=dt, projs=((o, i, r, (0, 0)),), batch=False) for dt in DTYPES for o, i in MERGE_SHAPES for r in MERGE_RANKS]
    return specs + [dict(name=f'mbatch_{dt}', dt=dt, projs=BATCH_TABLE, batch=True) for dt in DTYPES]


def merge_branches(spec):
    out = set()
    for o, i, r, off in spec['projs']:
        if not spec['batch']:
            out.add('single_stride' if o * i > 1024 * 256 else 'single_pass')
        elif o % 64 == 0 and i % 64 == 0:
            out |= {'batch_tiled', 'store4_fallback' if off[spec['dt'] == 'f32'] else 'store4_vector'}
        else:
            out.add('batch_elem_stride' if o * i > 256 * 256 else 'batch_elem_pass')
        if r == 0:
            out.add('batch_r0' if spec['batch'] else 'single_r0')
    return out


def make_merge(name, dt, projs, batch, device='cpu', seed=None):
    """per projection: W [out, in], A [r, in], B [out, r] contiguous with JUNK behind; dst = rows out .. 2 out of a [3 out + 2, in + 8] buffer of
    sentinels, dstT = columns out .. 2 out of an [in + 2, 3 out + 8] one, both shifted right by the slot offset"""
    g = _gen(device, seed_of(name) if seed is None else seed)
    T = DT[dt]
    c = SimpleNamespace(name=name, family='merge', dt=dt, T=T, batch=batch, device=device, inputs={}, expect={}, projs=[], same_bits=[], slot={})
    for n, (o, i, r, offs) in enumerate(projs):
        off = offs[dt == 'f32']
        rn = lambda *s: torch.randn(*s, generator=g, device=device)
        Wb, W = _tail(o * i, device)
        W.copy_(rn(o * i))
        W = W.view(o, i)
        c.inputs[f'W{n}'] = Wb
        Am = Bm = None
        s = 2.0 / max(r, 1)
        ref, f32v = W.double(), W.clone()
        if r:
            Ab, Am = _tail(r * i, device)
            Bb, Bm = _tail(o * r, device)
            Am.copy_(rn(r * i))
            Bm.copy_(rn(o * r))
            Am, Bm = Am.view(r, i), Bm.view(o, r)
            c.inputs[f'A{n}'], c.inputs[f'B{n}'] = Ab, Bb
            ref = ref + s * (Bm.double() @ Am.double())
            f32v = W + s * (Bm @ Am)
        if T == BF16:
            bound = 2 * float((rb(ref) - ref).abs().max()) + A.ulp_bf16(ref)
        else:
            bound = torch.full_like(ref, max(4 * float((f32v.double() - ref).abs().max()), 2.0 ** -22 * float(ref.abs().max())))
        shapes = dict(d=(3 * o + 2, i + 8), t=(i + 2, 3 * o + 8))
        at = dict(d=(slice(o, 2 * o), slice(off, off + i)), t=(slice(0, i), slice(o + off, 2 * o + off)))
        for k, v in (('d', ref), ('t', ref.t())):
            e = torch.full(shapes[k], SENTINEL, dtype=torch.float64, device=device)
            b = torch.zeros_like(e)
            e[at[k]], b[at[k]] = v, (bound if k == 'd' else bound.t())
            c.expect[f'{k}{n}'] = (e, b)
            c.slot[f'{k}{n}'] = (lambda sl: (lambda buf: buf[sl]))(at[k])
        c.same_bits.append((f'd{n}', f't{n}'))
        c.projs.append(SimpleNamespace(W=W, A=Am, B=Bm, s=s, r=r, o=o, i=i, shapes=shapes, at=at))
    return c


def run_merge(c, L):
    before = {k: b.clone() for k, b in c.inputs.items()}
    o, ents = {}, []
    for n, p in enumerate(c.projs):
        o[f'd{n}'] = torch.full(p.shapes['d'], SENTINEL, dtype=c.T, device=c.device)
        o[f't{n}'] = torch.full(p.shapes['t'], SENTINEL, dtype=c.T, device=c.device)
        ents.append((p.W, p.A, p.B, p.s, o[f'd{n}'][p.at['d']], o[f't{n}'][p.at['t']], p.r))
    if c.batch:
        L.lora_merge_batch(L.lora_table(ents, c.device))
    else:
        L.lora_merge(*ents[0])
    _sync(c)
    _unchanged(c, before)
    return o


# ================================================================== a4r_phm_build / a4r_phm_bwd
# name -> [(n, in, out, ldg - in, scratch rows - out)]; every PHMLinear of a case shares the case's one rule
PHM_CASES = {
    'phm_n1_64_16': [(1, 64, 16, 0, 0)], 'phm_n2_8_8': [(2, 8, 8, 0, 0)], 'phm_n4_8_8': [(4, 8, 8, 8, 0)], 'phm_n4_768_48': [(4, 768, 48, 0, 16)],
    'phm_n4_48_768': [(4, 48, 768, 16, 0)], 'phm_n8_768_64': [(8, 768, 64, 0, 0)], 'phm_n16_64_768': [(16, 64, 768, 8, 0)],
    'phm_pair': [(4, 768, 64, 0, 0), (4, 64, 768, 0, 0)], 'phm_trio': [(4, 768, 64, 8, 0), (4, 64, 768, 0, 0), (4, 768, 48, 0, 16)],
}
PHM_GAP = 3


def phm_branches(lins):
    out = {f'n{lins[0][0]}'}
    for n, i, o, dl, dr in lins:
        if (o // n) * (i // n) < 64:
            out.add('short_reduction')
        out |= ({'ldg_padded'} if dl else set()) | ({'out_padded'} if dr else set())
    if len(lins) > 1:
        out.add('shared_rule')
    if len(lins) > 2:
        out.add('shared_rule_3')
    return out


def phm_E(rule, wl, wr):
    """E [out, in] from rule [n, n, n], Wl [n, ip], Wr [n, oq]"""
    n = rule.shape[0]
    return torch.einsum('kab,kp,kq->bqap', rule, wl, wr).reshape(n * wr.shape[1], n * wl.shape[1])


def phm_terms(G, rule, wl, wr):
    """the terms of the three gradients, each [k, a, b, q, p]: (d rule sums over q, p; d Wl over a, b, q; d Wr over a, b, p)"""
    n, ip, oq = rule.shape[0], wl.shape[1], wr.shape[1]
    G5 = G.reshape(n, oq, n, ip).permute(2, 0, 1, 3)[None]                        # [1, a, b, q, p]
    r5, l5, q5 = rule[:, :, :, None, None], wl[:, None, None, None, :], wr[:, None, None, :, None]
    return (G5 * l5) * q5, (G5 * q5) * r5, (G5 * l5) * r5


def phm_grads(G, rule, wl, wr):
    tr, tl, tq = phm_terms(G, rule, wl, wr)
    return (tr.sum((3, 4)), tl.sum((1, 2, 3)), tq.sum((1, 2, 4))), (tr.abs().sum((3, 4)), tl.abs().sum((1, 2, 3)), tq.abs().sum((1, 2, 4)))


def make_phm(name, lins, device='cpu', seed=None):
    from adapter4rec_amd import _lib as REAL
    g = _gen(device, seed_of(name) if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    n = lins[0][0]
    segs, off = [('rule', n ** 3)], PHM_GAP
    for j, (n_, i, o, dl, dr) in enumerate(lins):
        assert n_ == n
        segs += [(f'wl{j}', n * (i // n)), (f'wr{j}', n * (o // n))]
    at = {}
    for k, sz in segs:
        at[k] = off
        off += sz + PHM_GAP
    params = torch.full((off,), JUNK, device=device)
    base = torch.full((off,), SENTINEL, device=device)
    for k, sz in segs:
        params[at[k]:at[k] + sz] = rn(sz) * (0.3 if k == 'rule' else 0.2)
        base[at[k]:at[k] + sz] = rn(sz) + 0.5
    c = SimpleNamespace(name=name, family='phm', lins=lins, n=n, device=device, at=at, size=dict(segs), base=base, inputs=dict(params=params), lin=[],
                        n_desc=len(lins))
    eoff, descs = PHM_GAP, []
    P = params.double()
    rule = P[at['rule']:at['rule'] + n ** 3].view(n, n, n)
    eg, bg = base.double(), torch.zeros(off, dtype=torch.float64, device=device)
    ag = torch.zeros_like(bg)
    for j, (n_, i, o, dl, dr) in enumerate(lins):
        ip, oq = i // n, o // n
        Gb = torch.full((o + dr + 1, i + dl), JUNK, device=device)
        Gb[:o, :i] = rn(o, i)
        c.inputs[f'G{j}'] = Gb
        wl, wr = P[at[f'wl{j}']:at[f'wl{j}'] + n * ip].view(n, ip), P[at[f'wr{j}']:at[f'wr{j}'] + n * oq].view(n, oq)
        E = phm_E(rule, wl, wr)
        E32 = phm_E(rule.float(), wl.float(), wr.float()).double()
        (dr_, dl_, dq_), (ar_, al_, aq_) = phm_grads(Gb[:o, :i].double(), rule, wl, wr)
        for k, v, a in (('rule', dr_, ar_), (f'wl{j}', dl_, al_), (f'wr{j}', dq_, aq_)):
            eg[at[k]:at[k] + v.numel()] += v.reshape(-1)
            ag[at[k]:at[k] + v.numel()] += a.reshape(-1)
        c.lin.append(SimpleNamespace(n=n, i=i, o=o, eoff=eoff, E=E, bound=max(4 * float((E32 - E).abs().max()), 2.0 ** -22 * float(E.abs().max())),
                                     G=Gb, rule=rule, wl=wl, wr=wr, k=('rule', f'wl{j}', f'wr{j}')))
        descs.append(REAL.PhmDesc(at['rule'], at[f'wl{j}'], at[f'wr{j}'], eoff, Gb.data_ptr(), Gb.stride(0), i, o, n, 0))
        eoff += o * i + PHM_GAP
    live = base != SENTINEL
    bg[live] = C_PHM * 2.0 ** -24 * (base.double().abs() + ag)[live]
    c.abs_grads = ag
    ee, be = torch.full((eoff,), SENTINEL, dtype=torch.float64, device=device), torch.zeros(eoff, dtype=torch.float64, device=device)
    for l in c.lin:
        ee[l.eoff:l.eoff + l.o * l.i], be[l.eoff:l.eoff + l.o * l.i] = l.E.reshape(-1), l.bound
    c.expect = dict(eff=(ee, be), grads=(eg, bg))
    c.descs, c.eff_len = descs, eoff
    return c


def run_phm(c, L):
    before = {k: b.clone() for k, b in c.inputs.items()}
    tab = L.desc_table(c.descs, c.device)
    eff = torch.full((c.eff_len,), SENTINEL, device=c.device)
    grads = c.base.clone()
    L.phm_build(c.inputs['params'], tab, c.n_desc, eff)
    L.phm_bwd(c.inputs['params'], tab, c.n_desc, grads)
    _sync(c)
    _unchanged(c, before)
    return dict(eff=eff, grads=grads)


# ================================================================== a4r_unpack_add
UNPACK_DESCS = ((1, 16, 16, 1.0), (16, 80, 96, 0.5), (130, 130, 136, -0.25), (300, 64, 64, 1.0))          # rows, cols, ld, alpha
UNPACK_MODES = ('true', 'small', 'offset0', 'offset2')
UNPACK_GRID = 64 * 256


def unpack_branches(mode):
    if mode.startswith('offset'):
        j = int(mode[-1])
        return {'table_offset', 'unpack_stride' if UNPACK_DESCS[j][0] * UNPACK_DESCS[j][1] > UNPACK_GRID else 'unpack_pass'}
    return {'unpack_stride', 'unpack_pass'} | ({'unpack_small_max'} if mode == 'small' else set())


def make_unpack(name, mode, device='cpu', seed=None):
    from adapter4rec_amd import _lib as REAL
    g = _gen(device, seed_of(name) if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    which = [int(mode[-1])] if mode.startswith('offset') else list(range(len(UNPACK_DESCS)))
    total = 7 + sum(r * cc + 5 for r, cc, _, _ in UNPACK_DESCS)
    base = rn(total)
    c = SimpleNamespace(name=name, family='unpack', mode=mode, device=device, base=base, inputs={}, which=which)
    e, b, e32 = base.double(), torch.zeros(total, dtype=torch.float64, device=device), base.clone()
    off, descs = 7, []
    for j, (r, cc, ld, alpha) in enumerate(UNPACK_DESCS):
        src = torch.full((r + 2, ld), JUNK, device=device)
        src[:r, :cc] = rn(r, cc)
        c.inputs[f'src{j}'] = src
        descs.append(REAL.AddDesc(src.data_ptr(), off, r, cc, ld, alpha))
        if j in which:
            sl = slice(off, off + r * cc)
            e[sl] += alpha * src[:r, :cc].double().reshape(-1)
            e32[sl] += alpha * src[:r, :cc].reshape(-1)
            b[sl] = max(4 * float((e32[sl].double() - e[sl]).abs().max()), 2.0 ** -22 * float(e[sl].abs().max()))
        off += r * cc + 5
    c.descs = descs
    c.max_elems = {'true': max(r * cc for r, cc, _, _ in UNPACK_DESCS), 'small': 1280}.get(mode, UNPACK_DESCS[which[0]][0] * UNPACK_DESCS[which[0]][1])
    c.expect = dict(target=(e, b))
    return c


def run_unpack(c, L):
    from adapter4rec_amd import _lib as REAL
    before = {k: b.clone() for k, b in c.inputs.items()}
    tab = L.desc_table(c.descs, c.device)
    target = c.base.clone()
    if c.mode.startswith('offset'):
        L.unpack_add(target, tab[c.which[0] * ctypes.sizeof(REAL.AddDesc):], 1, c.max_elems)
    else:
        L.unpack_add(target, tab, len(c.descs), c.max_elems)
    _sync(c)
    _unchanged(c, before)
    return dict(target=target)


# ================================================================== a4r_pack_matrices
PACK_H = (128, 256, 768, 1024)
# destination's live rows, live columns, rows_pad, cols_pad, dst_ld (0: contiguous), layout
PACK_DESTS = [(16, 64, 64, 64, 0, 0), (300, 257, 320, 320, 960, 0), (70, 130, 128, 192, 0, 0), (1, 1, 64, 64, 0, 0)] + \
             [(48, h, 64, h, 0, 1) for h in PACK_H] + [(h, 48, h, 64, 0, 2) for h in PACK_H]
PACK_TILED_MIN = 256 * 256


def pack_branches(dt, kernel):
    out = {'pack_' + kernel, 'pack_' + dt, 'pack_transpose', 'pack_plain', 'layout1', 'layout2', 'pack_ragged', 'pack_dst_ld'}
    return out | ({'tiled_stride'} if kernel == 'tiled' else {'elem_stride'})


def frag_map(layout, H_):
    """(row, column) of the [64, H] (layout 1) or [H, 64] (layout 2) matrix held at every index of its fragment-ordered copy, from the fragment
    description: H = NW waves x CW columns, KS = CW / 32 steps.  Layout 1: the 16 bytes of lane (kg, fr) in fragment (wave w, step s, row tile nt)
    hold row 16 nt + fr, columns w CW + 32 s + 8 kg + [0, 8), fragments in the order ((w KS + s) 4 + nt), lanes 16 kg + fr.  Layout 2: fragment
    (w, s, half h, step ks) holds row w CW + 32 s + 8 (fr >> 2) + 4 h + (fr & 3), columns 32 ks + 8 kg + [0, 8), order (((w KS + s) 2 + h) 2 + ks)."""
    NW = 4 if H_ == 128 else 8
    CW = H_ // NW
    KS = CW // 32
    idx = torch.arange(64 * H_)
    j, lane, frag = idx % 8, (idx // 8) % 64, idx // 512
    fr, kg = lane % 16, lane // 16
    if layout == 1:
        nt, ws = frag % 4, frag // 4
        s, w = ws % KS, ws // KS
        return 16 * nt + fr, w * CW + 32 * s + 8 * kg + j
    ks, h, ws = frag % 2, (frag // 2) % 2, frag // 4
    s, w = ws % KS, ws // KS
    return w * CW + 32 * s + 8 * (fr // 4) + 4 * h + fr % 4, 32 * ks + 8 * kg + j


def pack_specs():
    return [dict(name=f'pack_{dt}_{k}', dt=dt, kernel=k) for dt in DTYPES for k in ('tiled', 'elem')]


def make_pack(name, dt, kernel, device='cpu', seed=None):
    from adapter4rec_amd import _lib as REAL
    g = _gen(device, seed_of(name.replace('tiled', 'elem')) if seed is None else seed)                 # (both kernels see the same data)
    T = DT[dt]
    todo = [(d, tr) for d in PACK_DESTS for tr in (0, 1)]
    flat = torch.full((5 + sum(d[0] * d[1] + 5 for d, _ in todo),), JUNK, device=device)
    c = SimpleNamespace(name=name, family='pack', dt=dt, T=T, kernel=kernel, device=device, inputs=dict(flat=flat), expect={}, outs=[], descs=[])
    off = 5
    for n, ((lr, lc, rp, cp, ld, layout), tr) in enumerate(todo):
        v = torch.randn(lr, lc, generator=g, device=device)
        src = v.t().contiguous() if tr else v                          # what lies in flat: [rows, cols] = the destination's live block or its transpose
        flat[off:off + lr * lc] = src.reshape(-1)
        full = torch.zeros(rp, cp, dtype=torch.float64, device=device)
        full[:lr, :lc] = _round(v.double(), T)
        if layout:
            r_, c_ = frag_map(layout, cp if layout == 1 else rp)
            shape, e = (rp * cp + 16,), torch.full((rp * cp + 16,), SENTINEL, dtype=torch.float64, device=device)
            e[8:8 + rp * cp] = full[r_.to(device), c_.to(device)]
            view = (slice(8, 8 + rp * cp),)
        elif ld:
            shape, e = (rp + 3, ld), torch.full((rp + 3, ld), SENTINEL, dtype=torch.float64, device=device)
            e[:rp, 320:320 + cp] = full
            view = (slice(0, rp), slice(320, 320 + cp))
        else:
            shape, e = (rp + 3, cp), torch.full((rp + 3, cp), SENTINEL, dtype=torch.float64, device=device)
            e[:rp] = full
            view = (slice(0, rp), slice(None))
        c.expect[f'p{n}'] = (e, torch.zeros_like(e))
        c.outs.append((f'p{n}', shape, view))
        c.descs.append((off, src.shape[0], src.shape[1], rp, cp, tr | (layout << 1), ld))
        off += lr * lc + 5
    true_max = max(d[2] * d[3] for d in PACK_DESTS)
    c.max_elems = PACK_TILED_MIN if kernel == 'tiled' else min(true_max, PACK_TILED_MIN - 1)
    c.REAL = REAL
    return c


def run_pack(c, L):
    before = {k: b.clone() for k, b in c.inputs.items()}
    o, descs = {}, []
    for (nm, shape, view), d in zip(c.outs, c.descs):
        o[nm] = torch.full(shape, SENTINEL, dtype=c.T, device=c.device)
        dst = o[nm][view]
        descs.append(c.REAL.PackDesc(d[0], dst.data_ptr(), d[1], d[2], d[3], d[4], d[5], d[6]))
    L.pack_matrices(c.inputs['flat'], L.desc_table(descs, c.device), len(descs), c.max_elems, L.BF16 if c.T == BF16 else L.F32)
    _sync(c)
    _unchanged(c, before)
    return o


# ================================================================== the case table
FAMILY = dict(lora=(make_lora, run_lora), merge=(make_merge, run_merge), phm=(make_phm, run_phm), unpack=(make_unpack, run_unpack),
              pack=(make_pack, run_pack))
BRANCHES = {
    'lora': {'narrow', 'wide', 'single_tile', 'self_prefetch', 'ragged_round', 'full_rounds', 'chunk_empty', 'chunk_tail_only', 'chunk_unrolled',
             'chunk_unrolled_tail'} | {'bias_' + b for b in BIAS_MODES},
    'merge': {'single_stride', 'single_pass', 'single_r0', 'batch_tiled', 'batch_elem_stride', 'store4_vector', 'store4_fallback', 'batch_r0'},
    'phm': {'n1', 'n2', 'n4', 'n8', 'n16', 'short_reduction', 'ldg_padded', 'out_padded', 'shared_rule', 'shared_rule_3'},
    'unpack': {'unpack_stride', 'unpack_pass', 'unpack_small_max', 'table_offset'},
    'pack': {'pack_tiled', 'pack_elem', 'pack_bf16', 'pack_f32', 'pack_transpose', 'pack_plain', 'layout1', 'layout2', 'pack_ragged', 'pack_dst_ld',
             'tiled_stride', 'elem_stride'},
}


def specs(G):
    """family -> the specs of its cases at G workgroups of the LoRA kernel"""
    return dict(lora=lora_specs(G), merge=merge_specs(), phm=[dict(name=k, lins=v) for k, v in PHM_CASES.items()],
                unpack=[dict(name=f'unpack_{m}', mode=m) for m in UNPACK_MODES], pack=pack_specs())


def branches(family, spec, G):
    if family == 'lora':
        return lora_branches(spec['tiles'], spec['R'], spec['bias'], G)
    if family == 'merge':
        return merge_branches(spec)
    if family == 'phm':
        return phm_branches(spec['lins'])
    if family == 'unpack':
        return unpack_branches(spec['mode'])
    return pack_branches(spec['dt'], spec['kernel'])


def build(family, spec, device='cpu'):
    return FAMILY[family][0](**spec, device=device)


def run(c, L):
    return FAMILY[c.family][1](c, L)


G_CPU = 8
CASES = {s['name']: (fam, s) for fam, ss in specs(G_CPU).items() for s in ss}


@functools.lru_cache(maxsize=None)
def case(name):
    """the case on the CPU (G = 8), built once per process and shared read-only"""
    return build(*CASES[name])


def names(family):
    return [n for n, (f, _) in CASES.items() if f == family]
