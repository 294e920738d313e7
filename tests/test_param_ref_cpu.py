"""tests/param_ref.py proven on the CPU, before the kernels are held to it (tests/test_param_kernels_gpu.py):
  * its fp64 formulas equal independent formulations: the five separate products the fused LoRA backward replaced (tests/test_lora_fused_cpu.py),
    autograd through PHMLinear's own construction, sim_lib.frag_index for the fragment maps (which are bijections whose runs of 8 columns stay
    contiguous);
  * tests/sim_lib.py's fp32 restatements pass judge on every case, through the same strided buffers, sentinels and bounds as the kernels;
  * the integer LoRA cases are exact (t / dt exact in bf16, every |base| + sum |term| < 2^22), at G = 8 and at an MI355X's 16 x 769 rows; the random
    ones keep their near-tie share under 2 %;
  * every mutation that a wrong kernel could amount to FAILS its judge on a named case;
  * the constant of the PHM sums comes from the rule that set C_SUM (which does not cover them: C_PHM); the case table reaches every branch param_ref.BRANCHES lists.
"""
import ctypes
import math

import pytest
import torch

import param_ref as P
import sim_lib as S


def _judge(name, L):
    c = P.case(name)
    return c, P.judge(c, P.run(c, L))


# ------------------------------------------------------------------ the references against independent formulations
@pytest.mark.parametrize('name', ['lora_rand0_tG+1_8_8_5', 'lora_rand1_tG+1_16_15_9', 'lora_int_t3_8_1_8', 'lora_int_t2G+1_16_12_12'])
def test_lora_reference_equals_the_five_products(name):
    """t = x A^T with a column of ones, dt = (dq B_q) s + (dv B_v) s, dB_. = d.^T t, dA = dt^T x on the engine's 64-wide padded rank dimension
    (tests/test_lora_fused_cpu.py), in fp64 with t and dt rounded to bf16"""
    c = P.case(name)
    i, M, R, nb, H = c.inputs, c.M, c.R, c.nb, P.H
    X, Q, V = i['x'][:M, :H].double(), i['dqkv'][:M, :H].double(), i['dqkv'][:M, 2 * H:].double()
    Ap, Ba, Bb = (torch.zeros(P.RP, H, dtype=torch.float64) for _ in range(3))
    Ap[0:R], Ap[16:16 + R], Ba[0:R], Bb[16:16 + R] = i['A'][0:R].double(), i['A'][16:16 + R].double(), i['BTa'][0:R].double(), i['BTb'][16:16 + R].double()
    t = P.rb(X @ Ap.t())
    t[:, P.OC] = 1.0
    dt = P.rb(c.sq * (Q @ Ba.t()) + c.sv * (V @ Bb.t()))
    sBa, sBb, sA = Q.t() @ t, V.t() @ t, dt.t() @ X
    for k, v in (('dAq', sA[0:R]), ('dAv', sA[16:16 + R]), ('dBq', sBa[:, 0:nb]), ('dBv', sBb[:, 16:16 + nb]), ('dbq', sBa[:, P.OC]), ('dbv', sBb[:, P.OC])):
        assert float((c.ref[k] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k
    assert float(sA[R:16].abs().max() if R < 16 else 0) == 0 and float(c.ref['dAq'][c.rq:].abs().max() if c.rq < R else 0) == 0


def _effective_weight(rule, wl, wr):
    """PHMLinear's construction (the project's test of a4r_phm_build states it): W_left [n, ip, 1], W_right [n, 1, oq],
    E = (sum_k kron(rule[k], W_left[k] W_right[k]))^T"""
    n, ip, oq = rule.shape[0], wl.shape[1], wr.shape[1]
    w = torch.bmm(wl[:, :, None], wr[:, None, :])
    return (rule[:, :, None, :, None] * w[:, None, :, None, :]).reshape(n, n * ip, n * oq).sum(0).t()


@pytest.mark.parametrize('name', list(P.PHM_CASES))
def test_phm_reference_matches_autograd_of_the_construction(name):
    from adapter4rec_amd.model.modules import PHMLinear
    c = P.case(name)
    rule = c.lin[0].rule.clone().requires_grad_(True)
    leaves, Es = [rule], []
    for l in c.lin:
        m = PHMLinear(l.i, l.o, l.n)
        assert m.W_left.shape == (l.n, l.i // l.n, 1) and m.W_right.shape == (l.n, 1, l.o // l.n)
        wl, wr = l.wl.clone().requires_grad_(True), l.wr.clone().requires_grad_(True)
        leaves += [wl, wr]
        Es.append(_effective_weight(rule, wl, wr))
        assert float((Es[-1].detach() - l.E).abs().max()) < 1e-13 * max(1.0, float(l.E.abs().max()))
    want = torch.autograd.grad(Es, leaves, [l.G[:l.o, :l.i].double() for l in c.lin])
    e = c.expect['grads'][0] - c.base.double()
    keys = ['rule'] + [k for l in c.lin for k in l.k[1:]]
    for k, w in zip(keys, want):
        got = e[c.at[k]:c.at[k] + w.numel()]
        assert float((got - w.reshape(-1)).abs().max()) < 1e-11 * max(1.0, float(w.abs().max())), k


@pytest.mark.parametrize('H', [128, 256, 512, 768, 1024])
@pytest.mark.parametrize('layout', [1, 2])
def test_fragment_maps_are_bijections_with_contiguous_runs(layout, H):
    r, c = P.frag_map(layout, H)
    rows, cols = (64, H) if layout == 1 else (H, 64)
    assert int(r.min()) == 0 and int(r.max()) == rows - 1 and int(c.min()) == 0 and int(c.max()) == cols - 1
    flat = r * cols + c
    assert torch.equal(flat.sort().values, torch.arange(64 * H))                         # onto [0, rows_pad cols_pad), one to one
    runs_r, runs_c = r.view(-1, 8), c.view(-1, 8)
    assert bool((runs_r == runs_r[:, :1]).all()) and bool((runs_c == runs_c[:, :1] + torch.arange(8)).all()) and bool((runs_c[:, 0] % 8 == 0).all())
    fwd = S.frag_index(layout, rows, cols)                                               # the forward map of the simulator: the inverse of this one
    assert torch.equal(fwd[r, c], torch.arange(64 * H))


# ------------------------------------------------------------------ the simulated engine under the kernels' bounds
@pytest.mark.parametrize('name', list(P.CASES))
def test_sim_lib_passes_judge(name):
    c, (figures, fails) = _judge(name, S)
    print('SIM ' + P.table_row(c, figures))
    assert set(figures) == set(c.expect) and not fails, (name, fails)


def test_judge_sees_one_wrong_bit_outside_a_slot():
    c = P.case('merge_bf16_72x40_r8')
    got = P.run(c, S)
    got['d0'][0, 0] = 0.0                                       # a sentinel row above the slot
    assert any('must be exact' in f for f in P.judge(c, got)[1])
    got = P.run(c, S)
    got['t0'][3, 72 + 5] += 0.5
    assert any('transposed' in f for f in P.judge(c, got)[1])


# ------------------------------------------------------------------ the integer cases are exact; the random ones have few near ties
@pytest.mark.parametrize('name', P.names('lora'))
def test_lora_case_properties(name):
    c = P.case(name)
    if c.kind == 'int':
        exact, mag = P.lora_exactness(c)
        assert exact and mag < 2.0 ** 22, (exact, mag)
        assert all(float(b.max()) == 0 for _, b in c.expect.values())
    else:
        print(f'NEAR {name}: {c.near_share:.4%} of the live (row, rank) pairs')
        assert 0 <= c.near_share <= 0.02


@pytest.mark.parametrize('R,rq,rv', P.LORA_FORMS)
def test_integer_cases_stay_exact_at_the_largest_gpu_size(R, rq, rv):
    """3 G + 1 tiles at G = 256: 12 304 rows"""
    c = P.make_lora(f'lora_int_t3G+1_{R}_{rq}_{rv}', 3 * P.G_NOMINAL + 1, R, rq, rv, 'int', 'col')
    exact, mag = P.lora_exactness(c)
    print(f'EXACT {c.name}: M {c.M}, largest |base| + sum |term| {mag:.0f}, |t| <= {max(float(v.abs().max()) for v in c.t.values()):.1f}')
    assert exact and mag < 2.0 ** 22


# ------------------------------------------------------------------ mutation checks: each slip, applied to the restatement, fails its judge
class Mutant:
    """sim_lib with one function replaced"""
    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(S, k)


def _lora_mut(mut):
    def f(x, dqa, dqb, Aa, Ab, BTa, BTb, sa, sb, dAa, dAb, dBa, dBb, ba, bb, M, rank_rows=8):
        rows = torch.arange(M)
        if mut == 'drop_tile':
            t0 = 16 * ((M // 16) // 2)
            rows = torch.cat([rows[:t0], rows[t0 + 16:]])
        if mut == 'double_last':
            rows = torch.cat([rows, rows[-16:]])
        if mut == 'swap_qv':
            Aa, Ab = Ab, Aa
        if mut == 'dt_unscaled':
            sa = sb = 1.0
        if mut == 'bias_row':
            S.lora_bwd_fused(x[rows], dqa[rows], dqb[rows], Aa, Ab, BTa, BTb, sa, sb, dAa, dAb, dBa, dBb, None, None, len(rows), rank_rows=rank_rows)
            if ba is not None:
                dBa[:, rank_rows - 1] += dqa[:M].float().sum(0)
            if bb is not None:
                dBb[:, rank_rows - 1] += dqb[:M].float().sum(0)
            return
        if mut == 'db_stride':
            ta, tb = torch.zeros(x.shape[1], rank_rows), torch.zeros(x.shape[1], rank_rows)
            S.lora_bwd_fused(x[rows], dqa[rows], dqb[rows], Aa, Ab, BTa, BTb, sa, sb, dAa, dAb, ta, tb, ba, bb, len(rows), rank_rows=rank_rows)
            fit = dBa.shape[0] * dBa.stride(0) // dAa.stride(0) - 1                     # the rows that land inside the scratch at stride lda
            torch.as_strided(dBa, (fit, rank_rows), (dAa.stride(0), 1), dBa.storage_offset()).add_(ta[:fit])
            torch.as_strided(dBb, (fit, rank_rows), (dAa.stride(0), 1), dBb.storage_offset()).add_(tb[:fit])
            return
        S.lora_bwd_fused(x[rows], dqa[rows], dqb[rows], Aa, Ab, BTa, BTb, sa, sb, dAa, dAb, dBa, dBb, ba, bb, len(rows), rank_rows=rank_rows)
    return Mutant(lora_bwd_fused=f)


def _merge_mut(mut):
    def f(W, A, B, s, dst, dstT, r):
        k = r - 1 if mut == 'r_minus_1' else r
        w = W.float() + (s * (B[:, :k].float() @ A[:k].float()) if k > 0 else 0)
        if mut == 's_on_w':
            w = s * (W.float() + (B.float() @ A.float() if r else 0))
        dst.copy_(w.to(dst.dtype))
        dstT.copy_((w.reshape(dstT.shape) if mut == 'flat_transpose' else w.t()).to(dstT.dtype))
    return Mutant(lora_merge=f, lora_merge_batch=lambda tab: [f(*e) for e in tab])


def _phm_mut(mut):
    def parts(params, d):
        rule, wl, wr = S._phm_E(params, d)
        return (rule.transpose(1, 2) if mut == 'rule_ba' else rule), wl, wr

    def build(params, desc_dev, n_desc, eff):
        for d in S._parse(desc_dev, S.PhmDesc, n_desc):
            rule, wl, wr = parts(params, d)
            E = torch.einsum('kab,kp,kq->bpaq' if mut == 'ip_oq' else 'kab,kp,kq->bqap', rule, wl, wr)
            eff[d.out_off:d.out_off + d.in_f * d.out_f] = E.reshape(-1)

    def bwd(params, desc_dev, n_desc, grads):
        for d in S._parse(desc_dev, S.PhmDesc, n_desc):
            n, ip, oq = d.n, d.in_f // d.n, d.out_f // d.n
            rule, wl, wr = parts(params, d)
            ldg = d.in_f if mut == 'ldg_data' else d.ldg
            G = torch.as_strided(S._f32_at(d.G, (d.out_f - 1) * d.ldg + d.in_f), (d.out_f, d.in_f), (ldg, 1))
            G = G.reshape(n, ip, n, oq).permute(0, 3, 2, 1) if mut == 'ip_oq' else G.reshape(n, oq, n, ip)
            dr = torch.einsum('bqap,kp,kq->kab', G, wl, wr)
            grads[d.rule_off:d.rule_off + n ** 3] += (dr.transpose(1, 2) if mut == 'rule_ba' else dr).reshape(-1)
            grads[d.wl_off:d.wl_off + n * ip] += torch.einsum('bqap,kab,kq->kp', G, rule, wr).reshape(-1)
            grads[d.wr_off:d.wr_off + n * oq] += torch.einsum('bqap,kab,kp->kq', G, rule, wl).reshape(-1)
    return Mutant(phm_build=build, phm_bwd=bwd)


def _unpack_mut(mut):
    def f(target, desc_dev, n_desc, max_elems):
        for d in S._parse(desc_dev, S.AddDesc, n_desc):
            ld = d.cols if mut == 'ld_cols' else d.ld
            src = torch.as_strided(S._f32_at(d.src, (d.rows - 1) * d.ld + d.cols), (d.rows, d.cols), (ld, 1)).reshape(-1)
            n = min(src.numel(), P.UNPACK_GRID) if mut == 'first_pass' else src.numel()
            target.view(-1)[d.dst_off:d.dst_off + n] += d.alpha * src[:n]
    return Mutant(unpack_add=f)


def _pack_mut(mut):
    def f(flat, desc_dev, n_desc, max_elems, dtype):
        tdt = torch.bfloat16 if dtype == S.BF16 else torch.float32
        for d in S._parse(desc_dev, S.PackDesc, n_desc):
            src = flat[d.src_off:d.src_off + d.rows * d.cols].view(d.rows, d.cols)
            src = src.t() if d.transpose & 1 else src
            layout = d.transpose >> 1
            ld = d.cols_pad if (layout or mut == 'no_ld') else (d.dst_ld or d.cols_pad)
            n = (d.rows_pad - 1) * ld + d.cols_pad
            dst = torch.frombuffer((ctypes.c_char * (n * (2 if dtype == S.BF16 else 4))).from_address(d.dst), dtype=tdt).as_strided((d.rows_pad, d.cols_pad), (ld, 1))
            if layout:
                full = torch.zeros(d.rows_pad, d.cols_pad, dtype=tdt)
                full[:src.shape[0], :src.shape[1]] = src.to(tdt)
                idx = S.frag_index(3 - layout, d.cols_pad, d.rows_pad).t() if mut == 'layout_swap' else S.frag_index(layout, d.rows_pad, d.cols_pad)
                dst.view(-1)[idx.reshape(-1)] = full.view(-1)
                continue
            if mut != 'no_pad':
                dst.zero_()
            dst[:src.shape[0], :src.shape[1]] = src.to(tdt)
    return Mutant(pack_matrices=f)


MUTATIONS = [
    (_lora_mut, 'drop_tile', 'one 16-row tile dropped', ['lora_int_t3G+1_8_8_5', 'lora_int_t2G_16_12_12', 'lora_int_t2_8_1_8', 'lora_rand0_tG+1_16_15_9']),
    (_lora_mut, 'double_last', 'the last tile counted twice', ['lora_int_tG+1_8_8_5', 'lora_int_t1_16_15_9', 'lora_int_t3G+1_16_12_12', 'lora_rand1_tG+1_8_1_8']),
    (_lora_mut, 'swap_qv', 'ranks q / v swapped', ['lora_int_t5_8_8_5', 'lora_int_t5_16_15_9']),
    (_lora_mut, 'dt_unscaled', 'dt left unscaled', ['lora_int_t3_8_8_5', 'lora_rand0_tG+1_16_12_12']),
    (_lora_mut, 'bias_row', 'the bias sum in the wrong rank row', ['lora_int_t1_8_8_5', 'lora_int_tG_16_12_12', 'lora_int_t3_16_15_9']),
    (_lora_mut, 'db_stride', 'dB written at stride lda', ['lora_int_t2_8_8_5', 'lora_int_tG-1_16_12_12']),
    (_merge_mut, 'flat_transpose', 'the transpose of a non-square slot', ['merge_bf16_72x40_r8', 'merge_f32_72x40_r0', 'mbatch_bf16']),
    (_merge_mut, 's_on_w', 's applied to W too', ['merge_bf16_192x192_r8', 'merge_f32_768x768_r16', 'mbatch_f32']),
    (_merge_mut, 'r_minus_1', 'r - 1 ranks summed', ['merge_bf16_768x768_r1', 'merge_bf16_72x40_r16', 'merge_f32_192x192_r12', 'mbatch_bf16']),
    (_phm_mut, 'rule_ba', 'rule[k][b][a] for rule[k][a][b]', ['phm_n2_8_8', 'phm_n16_64_768', 'phm_trio']),
    (_phm_mut, 'ip_oq', 'ip and oq swapped', ['phm_n4_768_48', 'phm_n8_768_64', 'phm_pair']),
    (_phm_mut, 'ldg_data', 'the ldg padding read as data', ['phm_n4_8_8', 'phm_n4_48_768', 'phm_n16_64_768', 'phm_trio']),
    (_unpack_mut, 'first_pass', 'the first 16 384 elements only', ['unpack_true', 'unpack_small', 'unpack_offset2']),
    (_unpack_mut, 'ld_cols', 'ld taken as cols', ['unpack_true', 'unpack_offset2']),
    (_pack_mut, 'no_pad', 'the zero padding skipped', ['pack_bf16_tiled', 'pack_f32_elem']),
    (_pack_mut, 'layout_swap', 'layouts 1 and 2 exchanged', ['pack_bf16_elem', 'pack_f32_tiled']),
    (_pack_mut, 'no_ld', 'dst_ld ignored', ['pack_bf16_tiled', 'pack_f32_elem']),
]


@pytest.mark.parametrize('mk,mut,what,name', [(mk, mut, what, n) for mk, mut, what, ns in MUTATIONS for n in ns], ids=lambda v: v if isinstance(v, str) and ' ' not in v else '')
def test_mutation_fails_its_judge(mk, mut, what, name):
    c, (figures, fails) = _judge(name, mk(mut))
    print(f'MUTANT {what} on {name}: {fails[:2]}')
    assert fails, (what, name, 'passed every bound')


# ------------------------------------------------------------------ the constant of the atomically flushed PHM sums
def phm_sum_ratio(c, seed=0):
    """adapter_ln_ref.colsum_ratio's rule on the PHM sums: every term in fp32 (both products rounded), added one after the other in a shuffled
    order onto the base; the worst |sum - (base + ref)| / (2^-24 (|base| + sum |term|)) per gradient"""
    gen = torch.Generator().manual_seed(seed)
    acc = c.base.clone()
    for l in c.lin:
        terms = P.phm_terms(l.G[:l.o, :l.i], l.rule.float(), l.wl.float(), l.wr.float())          # fp32 throughout
        for k, t, dims in zip(l.k, terms, ((0, 1, 2, 3, 4), (0, 4, 1, 2, 3), (0, 3, 1, 2, 4))):
            t = t.permute(dims)
            nout = l.n ** 3 if k == 'rule' else t.shape[0] * t.shape[1]
            t = t.reshape(nout, -1)
            sl = acc[c.at[k]:c.at[k] + nout]
            for j in torch.randperm(t.shape[1], generator=gen).tolist():
                sl += t[:, j]
    want, _ = c.expect['grads']
    unit = 2.0 ** -24 * (c.base.double().abs() + c.abs_grads)
    out = {}
    for k, off in c.at.items():
        r = ((acc.double() - want).abs() / unit)[off:off + c.size[k]]
        kind = k.rstrip('0123456789')
        out[kind] = max(out.get(kind, 0.0), float(r.max()))
    return out


def test_c_sum_does_not_cover_the_phm_sums_and_c_phm_does():
    """4 x the worst ratio of the fp32 restatement exceeds C_SUM (sums of up to 12 288 three-factor terms, one after the other, onto bases that
    outweigh them): the PHM family's constant is that figure rounded up to a power of two"""
    worst = {}
    for name in P.PHM_CASES:
        r = phm_sum_ratio(P.case(name))
        print(f'PHMSUM {name}: ' + ' '.join(f'{k} {v:.2f}' for k, v in r.items()))
        for k, v in r.items():
            if v > worst.get(k, (0.0, ''))[0]:
                worst[k] = (v, name)
    print(f'PHMSUM worst: {worst}')
    top = 4 * max(v for v, _ in worst.values())
    assert P.C_SUM < top <= P.C_PHM and P.C_PHM == 2.0 ** math.ceil(math.log2(top)), (top, worst)


# ------------------------------------------------------------------ every listed branch has a case
@pytest.mark.parametrize('G', [P.G_CPU, P.G_NOMINAL])
def test_every_branch_has_a_case(G):
    for fam, ss in P.specs(G).items():
        seen = set().union(*(P.branches(fam, s, G) for s in ss))
        want = set(P.BRANCHES[fam])
        if G < 16:                       # fewer than 4 slices per reduction chunk: the unrolled loop needs the real machine's workgroup count
            want -= {'chunk_unrolled', 'chunk_unrolled_tail'}
        assert want <= seen, (fam, want - seen)
        assert seen <= set(P.BRANCHES[fam]) | {'batch_elem_pass'}, seen - set(P.BRANCHES[fam])
    labs = [P.tiles_of(l, G) for l in P.TILE_LABELS]
    assert len(set(labs)) == len(labs) and min(labs) == 1
