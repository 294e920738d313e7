"""GPU: the input side of both encoders -- a4r_embed_ln, a4r_embed_bwd, a4r_vit_assemble, a4r_patchify -- against plain fp64
restatements computed on the CPU from the same inputs.

bf16 inputs are pre-rounded, so only the accumulation order and the output rounding separate kernel and reference.  Every
tolerance is an error bound written out next to the check (u = 2^-24, the fp32 unit roundoff); each check prints the largest
error-to-bound ratio it saw (`RATIO <what> <ratio>`, visible under `pytest -s`).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def dev():
    return torch.device('cuda:0')


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0, offset=0.0):
    """Host tensor: randn * scale + offset, rounded to dtype."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + offset).to(dtype)


def report(what, err, bound):
    """Assert err <= bound elementwise; print the largest ratio."""
    err, bound = err.double(), bound.double()
    bad = err > bound
    ratio = float((err / bound).max()) if err.numel() else 0.0
    print(f'RATIO {what} {ratio:.3e}')
    assert not bad.any(), (f'{what}: {int(bad.sum())}/{bad.numel()} outside the bound, first at {bad.nonzero()[0].tolist()}: '
                           f'err {float(err[bad][0]):.3e} bound {float(bound[bad][0]):.3e}')
    return ratio


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (the larger one at a power of two)."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def title_ids(n_items, S, V, pad, seed, ld=None, negatives=True):
    """ids || mask rows [n_items, 2S] (row stride ld >= 2S: the columns behind 2S hold other valid ids).  Titles cover pads inside
    and at the end of a title, an all-pad title, the last vocabulary row and (negatives) soft-prompt ids -(r + 1), also where the
    original token was a pad."""
    g = torch.Generator().manual_seed(seed)
    ld = ld or 2 * S
    big = torch.randint(0, V, (n_items, ld), generator=g)
    ids = big[:, :S]
    ids[torch.rand(n_items, S, generator=g) < 0.15] = pad
    ids[0] = pad                                          # a title made only of pads
    if n_items > 1 and S > 1:
        ids[1, S // 2:] = pad                             # pads at the end
    if n_items > 2 and S > 4:
        ids[2, 1:S - 1:3] = pad                           # pads inside
    k = int(torch.randint(S, n_items * S, (1,), generator=g))      # (not in the all-pad title 0)
    ids[k // S, k % S] = V - 1
    if negatives:
        neg = torch.rand(n_items, S, generator=g) < 0.1
        neg[0, :min(S, 3)] = True                         # redirected pads
        ids[neg] = -torch.randint(0, V, (int(neg.sum()),), generator=g) - 1
    big[:, S:2 * S] = (ids != pad).long()
    return big[:, :2 * S]


def to_dev(t):
    """Device copy of a 2-D host view that keeps its row stride (Tensor.to would compact a strided view)."""
    full = torch.as_strided(t, (t.shape[0], t.stride(0)), (t.stride(0), 1))
    return full.to(dev())[:, :t.shape[1]]


def ref_positions(raw, roberta, pad):
    """HF position ids: BERT arange(S); RoBERTa cumsum(id != pad) * (id != pad) + pad, a negative id counting as a pad."""
    n, S = raw.shape
    if roberta:
        m = ((raw != pad) & (raw >= 0)).long()
        return torch.cumsum(m, 1) * m + pad
    return torch.arange(S).expand(n, S)


def word_rows(raw):
    return torch.where(raw < 0, -raw - 1, raw)


# ------------------------------------------------------------------ a4r_embed_bwd
def embed_bwd_ref(raw, g64, V, P, roberta, pad):
    """fp64 nn.Embedding(padding_idx) backward: (sum, sum of |g|, number of adds) per table element."""
    H = g64.shape[1]
    wid = word_rows(raw).reshape(-1)
    pid = ref_positions(raw, roberta, pad).reshape(-1)
    out = {}
    for name, idx, keep, rows in (('word', wid, wid != pad, V),
                                  ('pos', pid, (pid != pad) if roberta else torch.ones_like(pid, dtype=torch.bool), P)):
        i, gk = idx[keep], g64[keep]
        s = torch.zeros(rows, H, dtype=torch.float64).index_add_(0, i, gk)
        a = torch.zeros(rows, H, dtype=torch.float64).index_add_(0, i, gk.abs())
        n = torch.bincount(i, minlength=rows).double()[:, None].expand(rows, H)
        out[name] = (s, a, n)
    return out


def check_accumulated(got, init, s, a, n, what):
    """got = init + the n adds of s, in some order of fp32 atomic adds: n roundings of partial sums no larger than |init| + a, so
    |got - (init + s)| <= gamma_n * (|init| + a), gamma_n = n u / (1 - n u) (recursive summation, init counted as a term).  A row
    no token touches (n = 0) keeps its starting bits."""
    got = got.cpu()
    untouched = n == 0
    assert torch.equal(got[untouched], init[untouched]), f'{what}: an element no token adds into changed'
    gam = n * U32 / (1 - n * U32)
    err = (got.double() - (init.double() + s)).abs()
    t = ~untouched
    return report(what, err[t], gam[t] * (init.double().abs() + a)[t] + 1e-300)


def run_embed_bwd(ids_h, dpre_h, V, P, roberta, pad, S, which=('word', 'pos'), ldd_pad=0, seed=0):
    from adapter4rec_amd import _lib as L
    n_items, H = ids_h.shape[0], dpre_h.shape[1]
    if ldd_pad:                                           # strided dpre view: the columns behind H hold large values
        big = torch.full((dpre_h.shape[0], H + ldd_pad), 1e3, dtype=dpre_h.dtype)
        big[:, :H] = dpre_h
        dpre = big.to(dev())[:, :H]
        assert dpre.stride(0) == H + ldd_pad
    else:
        dpre = dpre_h.to(dev())
    init = {'word': rnd(V, H, seed=seed + 1), 'pos': rnd(P, H, seed=seed + 2)}
    tabs = {k: (init[k].to(dev()) if k in which else None) for k in init}
    L.embed_bwd(to_dev(ids_h), dpre, tabs['word'], tabs['pos'], n_items, S, roberta=roberta, pad_id=pad)
    torch.cuda.synchronize()
    return init, tabs


def n_pos_rows(S, roberta, pad):
    return S + pad + 1 if roberta else S


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
@pytest.mark.parametrize('S', [1, 30, 64, 512])
@pytest.mark.parametrize('H', [64, 128, 200, 256, 768, 1024])
def test_embed_bwd_vs_fp64(H, S, roberta, dt):
    """Both tables at once; ids || mask rows (ld_ids = 2S); a small vocabulary so that most rows take many adds.  Bound: see
    check_accumulated."""
    pad = 1 if roberta else 0
    V = 97
    n_items = max(3, 4096 // S)
    ids = title_ids(n_items, S, V, pad, seed=H * 7 + S)
    dpre = rnd(n_items * S, H, dtype=DT[dt], seed=H + S)  # non-zero on pad rows too
    P = n_pos_rows(S, roberta, pad) + 3
    init, tabs = run_embed_bwd(ids, dpre, V, P, roberta, pad, S, seed=H)
    ref = embed_bwd_ref(ids[:, :S], dpre.double(), V, P, roberta, pad)
    for k in ('word', 'pos'):
        check_accumulated(tabs[k], init[k], *ref[k], f'embed_bwd {k} H={H} S={S} roberta={roberta} {dt}')


@pytest.mark.parametrize('which', [('word',), ('pos',), ('word', 'pos')], ids=['word', 'pos', 'both'])
@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_bwd_one_table_strided(which, roberta):
    """One table alone (the other NULL) or both; ld_ids > 2S; a strided dpre view (ldd > H)."""
    pad = 1 if roberta else 0
    S, H, V, n_items = 30, 256, 61, 40
    ids = title_ids(n_items, S, V, pad, seed=11, ld=2 * S + 7)
    assert ids.stride(0) == 2 * S + 7
    dpre = rnd(n_items * S, H, seed=12)
    P = n_pos_rows(S, roberta, pad)
    assert to_dev(ids).stride(0) == 2 * S + 7
    init, tabs = run_embed_bwd(ids, dpre, V, P, roberta, pad, S, which=which, ldd_pad=24, seed=13)
    ref = embed_bwd_ref(ids[:, :S], dpre.double(), V, P, roberta, pad)
    for k in ('word', 'pos'):
        if k in which:
            check_accumulated(tabs[k], init[k], *ref[k], f'embed_bwd {k} of {which} roberta={roberta}')


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_bwd_hot_rows(roberta, dt):
    """Contention: 4096 titles all starting with the same CLS id and each position row taking up to 4096 atomic adds, over a
    vocabulary of 64 rows.  Atomics need not repeat their bits, so two runs are each held to the bound, not to each other."""
    pad = 1 if roberta else 0
    S, H, V, n_items = 30, 128, 64, 4096
    ids = title_ids(n_items, S, V, pad, seed=21, negatives=False)
    ids[:, 0] = 2                                         # the CLS id of every title
    ids[:, S:2 * S] = (ids[:, :S] != pad).long()
    dpre = rnd(n_items * S, H, dtype=DT[dt], seed=22)
    P = n_pos_rows(S, roberta, pad)
    ref = embed_bwd_ref(ids[:, :S], dpre.double(), V, P, roberta, pad)
    assert float(ref['pos'][2].max()) >= 4000 and float(ref['word'][2][2].max()) >= 4096
    for rep in range(2):
        init, tabs = run_embed_bwd(ids, dpre, V, P, roberta, pad, S, seed=23)
        for k in ('word', 'pos'):
            check_accumulated(tabs[k], init[k], *ref[k], f'embed_bwd hot {k} roberta={roberta} {dt} run {rep}')


@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_bwd_padding_rows(roberta):
    """nn.Embedding(padding_idx) as HF declares it: word row pad_id never receives a gradient (BERT and RoBERTa), nor does
    RoBERTa's position row pad_id; BERT's position rows all do.  A negative id -(r + 1) standing where the title had a pad still
    adds into word row r.  dpre is non-zero on every pad row."""
    pad = 1 if roberta else 0
    S, H, V, n_items = 30, 64, 50, 16
    ids = title_ids(n_items, S, V, pad, seed=31)
    ids[0, 0] = -(7 + 1)                                  # title 0 is all pads: a redirected pad
    ids[0, S:2 * S] = 0
    dpre = rnd(n_items * S, H, seed=32, offset=1.0)
    P = n_pos_rows(S, roberta, pad)
    init, tabs = run_embed_bwd(ids, dpre, V, P, roberta, pad, S, seed=33)
    word, pos = tabs['word'].cpu(), tabs['pos'].cpu()
    assert torch.equal(word[pad], init['word'][pad]), f'word row pad_id={pad} received a gradient'
    if roberta:
        assert torch.equal(pos[pad], init['pos'][pad]), f'position row pad_id={pad} received a gradient'
        assert not torch.equal(pos[pad + 1], init['pos'][pad + 1])
    else:
        assert not torch.equal(pos[:S], init['pos'][:S]) and all(not torch.equal(pos[s], init['pos'][s]) for s in range(S))
    assert not torch.equal(word[7], init['word'][7])      # the redirected pad reached its row


@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_bwd_position_ids_exact(roberta):
    """Decode every token's position row from the gradient: token s of one title carries 2^s in every column (sums of distinct
    powers of two are exact), so dpos[p] names the tokens that landed on row p."""
    pad = 1 if roberta else 0
    S, H = 20, 64
    raw = torch.tensor([[2, 5, pad, 9, pad, pad, 3, -4, pad, 7, 8, -(pad + 1), pad, 4, 4, pad, 6, 2, pad, pad]])
    ids = torch.cat([raw, (raw != pad).long()], 1)
    dpre = (2.0 ** torch.arange(S, dtype=torch.float64))[:, None].expand(S, H).float().contiguous()
    from adapter4rec_amd import _lib as L
    P = n_pos_rows(S, roberta, pad)
    dpos = torch.zeros(P, H, device=dev())
    L.embed_bwd(ids.to(dev()), dpre.to(dev()), None, dpos, 1, S, roberta=roberta, pad_id=pad)
    got = dpos.cpu()[:, 0].long()
    pid = ref_positions(raw, roberta, pad)[0]
    exp = torch.zeros(P, dtype=torch.long)
    for s in range(S):
        if not (roberta and int(pid[s]) == pad):
            exp[int(pid[s])] += 1 << s
    assert torch.equal(got, exp), (got.tolist(), exp.tolist())
    assert torch.equal(dpos.cpu(), dpos.cpu()[:, :1].expand(P, H))


# ------------------------------------------------------------------ a4r_embed_ln
def embed_ln_ref(raw, word, pos, typ, gamma, beta, eps, roberta, pad):
    """fp64: x = word[id] + pos[pid] + type0, its LayerNorm and the per-element input scale |word| + |pos| + |type0|."""
    w, p = word.double()[word_rows(raw)], pos.double()[ref_positions(raw, roberta, pad)]
    t = typ.double()
    x = (w + p + t).reshape(-1, word.shape[1])
    absx = (w.abs() + p.abs() + t.abs()).reshape(-1, word.shape[1])
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean[:, None]) * rstd[:, None]
    y = xhat * gamma.double() + beta.double()
    return x, absx, mean, rstd, xhat, y


def ln_bounds(absx, rstd, xhat):
    """Error bounds of the fp32 two-pass row statistics.  A = max |word| + |pos| + |type0| of the row, c = A * rstd (the row's
    condition number).  The fp32 sum w + (p + t) errs by <= 2uA per element; a 16-term lane sum and a 6-level wave tree add
    <= 22u * mean|x|: |d mean| <= 25uA.  Deviations then err by <= 27uA, so (Cauchy-Schwarz: sum|d| <= sqrt(H sum d^2))
    rel. error of the variance <= 54uc + 23u and of rstd (half of it + rsqrt's own) <= u (27c + 16); taken as u (30c + 20)."""
    A = absx.max(-1).values
    c = A * rstd
    e_mean = 25 * U32 * A
    r_e = U32 * (30 * c + 20)
    e_xhat = U32 * 27 * c[:, None] + xhat.abs() * r_e[:, None]        # |d xhat| per element
    return A, c, e_mean, r_e, e_xhat


def embed_ln_case(H, S, roberta, V, n_items, seed, word_offset=0.0, word_scale=1.0, small_pos=False, negatives=True):
    pad = 1 if roberta else 0
    P = 514 if (roberta and S == 512) else n_pos_rows(S, roberta, pad) + 2
    ids = title_ids(n_items, S, V, pad, seed=seed, negatives=negatives)
    word = rnd(V, H, seed=seed + 1, scale=word_scale, offset=word_offset)
    ps = 0.01 if small_pos else 1.0
    pos, typ = rnd(P, H, seed=seed + 2, scale=ps), rnd(H, seed=seed + 3, scale=ps)
    gamma, beta = rnd(H, seed=seed + 4, scale=0.3, offset=1.0), rnd(H, seed=seed + 5, scale=0.3)
    return pad, ids, word, pos, typ, gamma, beta


def run_embed_ln(ids, word, pos, typ, gamma, beta, eps, t, S, roberta, pad, drop_p=0.0, seed=0):
    from adapter4rec_amd import _lib as L
    n_items, H = ids.shape[0], word.shape[1]
    rows = n_items * S
    out = torch.full((rows, H), 7.0, dtype=t, device=dev())
    pre = torch.full((rows, H), 7.0, dtype=t, device=dev())
    st = torch.full((rows, 2), 7.0, device=dev())
    km = torch.full((n_items, S), 7.0, device=dev())
    L.embed_ln(to_dev(ids), word.to(dev()), pos.to(dev()), typ.to(dev()), gamma.to(dev()), beta.to(dev()), eps, out, n_items, S,
               roberta=roberta, pad_id=pad, drop_p=drop_p, drop_site=999, drop_seed=seed, pre_out=pre, stats_out=st, key_mask_out=km)
    torch.cuda.synchronize()
    return out.cpu(), pre.cpu(), st.cpu(), km.cpu()


def check_embed_ln(got, ids, S, ref, gamma, beta, t, what):
    out, pre, st, km = got
    x, absx, mean, rstd, xhat, y = ref
    A, c, e_mean, r_e, e_xhat = ln_bounds(absx, rstd, xhat)
    assert torch.equal(km, ids[:, S:2 * S].float()), f'{what}: key_mask_out'
    report(f'{what} stats.mean', (st[:, 0].double() - mean).abs(), e_mean)
    report(f'{what} stats.rstd', (st[:, 1].double() - rstd).abs() / rstd, r_e)
    e_pre = 2 * U32 * absx                                # w + (p + t): two fp32 roundings
    e_y = gamma.double().abs() * e_xhat + 4 * U32 * (y.abs() + beta.double().abs())
    if t == torch.float32:
        report(f'{what} pre_out', (pre.double() - x).abs(), e_pre)
        report(f'{what} out', (out.double() - y).abs(), e_y)
    else:                                                 # at most one bf16 ulp from the fp64 value rounded once (+ the fp32 error)
        for name, g_, r_, e_ in (('pre_out', pre, x, e_pre), ('out', out, y, e_y)):
            r1 = r_.to(torch.bfloat16).double()
            report(f'{what} {name}', (g_.double() - r1).abs(), bf16_ulp(torch.maximum(r_.abs(), r1.abs())) + e_)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
@pytest.mark.parametrize('S', [1, 30, 512])
@pytest.mark.parametrize('H', [64, 128, 256, 768, 1024])
def test_embed_ln_outputs_vs_fp64(H, S, roberta, dt):
    """out, pre_out, stats_out and key_mask_out against fp64 (bounds: ln_bounds; out adds the gamma/beta products' roundings).
    RoBERTa at S = 512 reads a 514-row position table up to its last row (pid = 513 for a title without pads)."""
    t = DT[dt]
    V = 300
    n_items = max(4, 2048 // S)
    pad, ids, word, pos, typ, gamma, beta = embed_ln_case(H, S, roberta, V, n_items, seed=H + 3 * S + int(roberta))
    if roberta and S == 512:
        ids[3, :S] = torch.randint(2, V, (S,), generator=torch.Generator().manual_seed(1))
        ids[3, S:] = 1
        assert int(ref_positions(ids[:, :S], roberta, pad).max()) == 513
    eps = 1e-5 if roberta else 1e-12
    got = run_embed_ln(ids, word, pos, typ, gamma, beta, eps, t, S, roberta, pad)
    check_embed_ln(got, ids, S, embed_ln_ref(ids[:, :S], word, pos, typ, gamma, beta, eps, roberta, pad), gamma, beta, t,
                   f'embed_ln H={H} S={S} roberta={roberta} {dt}')


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_embed_ln_large_offset_rows(dt):
    """Word rows ~ 30 +- 0.02 under small position / type rows: a one-pass variance (E[x^2] - mean^2) keeps none of its digits
    here; the two-pass statistics stay inside ln_bounds (whose rstd bound grows with c = A * rstd ~ 1e3, still ~1e-4 of rstd)."""
    t = DT[dt]
    pad, ids, word, pos, typ, gamma, beta = embed_ln_case(768, 30, False, 50, 16, seed=41, word_offset=30.0, word_scale=0.02,
                                                          small_pos=True, negatives=False)
    got = run_embed_ln(ids, word, pos, typ, gamma, beta, 1e-12, t, 30, False, pad)
    ref = embed_ln_ref(ids[:, :30], word, pos, typ, gamma, beta, 1e-12, False, pad)
    assert float(ref[3].min()) > 20                       # std < 0.05 against a mean of 30
    check_embed_ln(got, ids, 30, ref, gamma, beta, t, f'embed_ln offset {dt}')


@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_ln_position_ids_exact(roberta):
    """pos[p] = p in every column, zero word / type rows: pre_out names the position row each token read."""
    pad = 1 if roberta else 0
    S, H, V, n_items = 40, 64, 30, 12
    ids = title_ids(n_items, S, V, pad, seed=51)
    P = n_pos_rows(S, roberta, pad)
    pos = torch.arange(P, dtype=torch.float32)[:, None].expand(P, H).contiguous()
    word, typ = torch.zeros(V, H), torch.zeros(H)
    _, pre, _, _ = run_embed_ln(ids, word, pos, typ, torch.ones(H), torch.zeros(H), 1e-12, torch.float32, S, roberta, pad)
    assert torch.equal(pre[:, 0].long().view(n_items, S), ref_positions(ids[:, :S], roberta, pad))


@pytest.mark.parametrize('roberta', [False, True], ids=['bert', 'roberta'])
def test_embed_ln_dropout_and_ln_bwd_round_trip(roberta):
    """Dropout at site 999 (the engine's): out == the no-dropout out * DropoutStream(seed).mask('rows', 999, ...) bit for bit in
    fp32; pre_out and stats_out do not depend on dropout.  Then the engine's backward chain (a4r_ln_bwd on pre_out, stats_out and
    the same dropout arguments) against the fp64 autograd of dropout(LN(x)).  Bound on dx: rstd * (r_e |dx| / rstd + 24uG
    + |m2| e_xhat + |xhat| (G max e_xhat + 22uGX)) + u |dx|, G = max|g|, g = dy * mask * gamma, m2 = mean(g xhat), X = max|xhat|.
    dgamma / dbeta: column sums over M rows in an unfixed order: gamma_M * sum|term| + sum |dy'| e_xhat."""
    from adapter4rec_amd import _lib as L
    from oracle.dropout_masks import DropoutStream
    S, H, n_items, p, seed = 30, 768, 9, 0.1, 1234
    pad, ids, word, pos, typ, gamma, beta = embed_ln_case(H, S, roberta, 200, n_items, seed=61)
    eps = 1e-12
    rows = n_items * S
    out0, pre0, st0, _ = run_embed_ln(ids, word, pos, typ, gamma, beta, eps, torch.float32, S, roberta, pad)
    out1, pre1, st1, _ = run_embed_ln(ids, word, pos, typ, gamma, beta, eps, torch.float32, S, roberta, pad, drop_p=p, seed=seed)
    mask = DropoutStream(seed).mask('rows', 999, torch.zeros(rows, H), p)
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    assert torch.equal(out1, out0 * mask), 'dropout output is not out * mask'
    assert torch.equal(pre1, pre0) and torch.equal(st1, st0)

    dy = rnd(rows, H, seed=62)
    dv = torch.full((rows, H), 7.0, device=dev())
    dg, db = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
    L.ln_bwd(dy.to(dev()), pre1.to(dev()), st1.to(dev()), gamma.to(dev()), dv, M=rows, dgamma=dg, dbeta=db,
             drop_p=p, drop_site=999, drop_seed=seed)
    torch.cuda.synchronize()
    x, absx, mean, rstd, xhat, y = embed_ln_ref(ids[:, :S], word, pos, typ, gamma, beta, eps, roberta, pad)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xr, (H,), gr, br, eps) * mask.double()
    dx_ref, dg_ref, db_ref = torch.autograd.grad(yr, [xr, gr, br], dy.double())
    _, _, _, r_e, e_xhat = ln_bounds(absx, rstd, xhat)
    dyp = dy.double() * mask.double()
    g = dyp * gamma.double()
    G, X = g.abs().max(-1).values[:, None], xhat.abs().max(-1).values[:, None]
    m2 = (g * xhat).mean(-1, keepdim=True)
    r = rstd[:, None]
    e_dx = (r_e[:, None] * dx_ref.abs() + r * (24 * U32 * G + m2.abs() * e_xhat + xhat.abs() * (G * e_xhat.max(-1, keepdim=True).values
                                                                                               + 22 * U32 * G * X)) + U32 * dx_ref.abs())
    report(f'ln_bwd dx roberta={roberta}', (dv.cpu().double() - dx_ref).abs(), e_dx)
    gM = rows * U32 / (1 - rows * U32)
    report(f'ln_bwd dgamma roberta={roberta}', (dg.cpu().double() - dg_ref).abs(),
           gM * (dyp * xhat).abs().sum(0) + (dyp.abs() * e_xhat).sum(0))
    report(f'ln_bwd dbeta roberta={roberta}', (db.cpu().double() - db_ref).abs(), gM * dyp.abs().sum(0) + 1e-300)


# ------------------------------------------------------------------ a4r_vit_assemble
def vit_case(n_items, n_keep, n_patches, H, t, keep, seed, ld_pad=0):
    g = torch.Generator().manual_seed(seed)
    ldp = H + ld_pad
    pbig = rnd(n_items * n_keep, ldp, dtype=t, seed=seed + 1)
    cls, pos = rnd(H, seed=seed + 2), rnd(1 + n_patches, H, seed=seed + 3)
    kidx = torch.stack([torch.randperm(n_patches, generator=g)[:n_keep] for _ in range(n_items)]).to(torch.int32) if keep else None
    return pbig, cls, pos, kidx


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('keep,n_keep', [(False, 49), (True, 1), (True, 12), (True, 49)], ids=['all', 'keep1', 'keep12', 'keepall'])
@pytest.mark.parametrize('ld_pad', [0, 24])
def test_vit_assemble_vs_fp64(dt, keep, n_keep, ld_pad):
    """[cls + pos[0]] ++ [patch_j + pos[1 + keep_j]] (keep order unsorted); fp32: the fp64 sum rounded once; bf16: the fp32 sum
    rounded once -- bit-equal.  ldp, ldo > H; tokens_out > n_keep + 1 leaves rows n_keep + 1 .. tokens_out - 1 of every item
    (and the columns behind H) at their sentinel."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    H, n_items, n_patches = 384, 5, 49
    pbig, cls, pos, kidx = vit_case(n_items, n_keep, n_patches, H, t, keep, seed=71 + n_keep, ld_pad=ld_pad)
    if keep:
        assert any(not bool((kidx[i, 1:] >= kidx[i, :-1]).all()) for i in range(n_items)) or n_keep == 1
    extra = 3
    T_out = n_keep + 1 + extra
    obig = torch.full((n_items * T_out, H + ld_pad), -77.0, dtype=t, device=dev())
    out = obig[:, :H]
    L.vit_assemble(pbig.to(dev())[:, :H], cls.to(dev()), pos.to(dev()), out, n_items, n_keep,
                   kidx.to(dev()) if keep else None, tokens_out=T_out)
    idx = kidx.long() if keep else torch.arange(n_keep).expand(n_items, n_keep)
    patches = pbig[:, :H].reshape(n_items, n_keep, H)
    if t == torch.float32:
        tok = torch.cat([(cls.double() + pos.double()[0]).expand(n_items, 1, H), patches.double() + pos.double()[1 + idx]], 1).float()
    else:
        tok = torch.cat([(cls + pos[0]).expand(n_items, 1, H), patches.float() + pos[1 + idx]], 1).to(t)
    got = obig.cpu().view(n_items, T_out, H + ld_pad)
    assert torch.equal(got[:, :n_keep + 1, :H], tok), 'vit_assemble tokens'
    assert (got[:, n_keep + 1:] == -77.0).all(), 'rows behind n_keep + 1 were written'
    assert (got[:, :, H:] == -77.0).all(), 'columns behind H were written'


def test_vit_assemble_rejects_before_launch():
    """H % 8, a misaligned pointer, tokens_out < n_keep + 1: A4R_EINVAL, nothing written.  (The buffers are large enough that even a
    launch would stay in bounds.)"""
    from adapter4rec_amd import _lib as L
    n_items, n_keep, H = 2, 4, 64
    pbig, cls, pos, _ = vit_case(n_items, n_keep, 16, H, torch.float32, False, seed=81)
    p, c, ps = pbig.to(dev()), cls.to(dev()), pos.to(dev())
    out = torch.full((n_items * (n_keep + 1) + 1, H), -5.0, device=dev())
    cases = {
        'H % 8': lambda: L.vit_assemble(p[:, :60], c[:60], ps[:, :60].contiguous(), out[:, :60], n_items, n_keep),
        'misaligned out': lambda: L.vit_assemble(p, c, ps, out.view(-1)[1:1 + (n_items * (n_keep + 1)) * H].view(-1, H), n_items, n_keep),
        'misaligned patches': lambda: L.vit_assemble(pbig.to(dev()).view(-1)[1:1 + (n_items * n_keep - 1) * H].view(-1, H), c, ps, out,
                                                     n_items, n_keep - 1),
        'tokens_out < n_keep + 1': lambda: L.vit_assemble(p, c, ps, out, n_items, n_keep, tokens_out=n_keep),
    }
    for what, call in cases.items():
        with pytest.raises(RuntimeError, match='invalid argument'):
            call()
        torch.cuda.synchronize()
        assert (out == -5.0).all(), f'{what}: output written'


# ------------------------------------------------------------------ a4r_patchify
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('P', [8, 16, 32])
@pytest.mark.parametrize('keep', [False, True])
def test_patchify_vs_unfold(P, C, dt, keep):
    """Non-square images (96 x 64), ldo > C P P: unfold of the normalised floats, bit-equal (bf16: rounded once), from the uint8
    and the fp32 source alike; the columns behind C P P keep their sentinel."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n, Hi, Wi = 3, 96, 64
    g = torch.Generator().manual_seed(P * 10 + C)
    u8 = torch.randint(0, 256, (n, Hi, Wi, C), generator=g, dtype=torch.uint8)
    f = ((u8.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    n_p = (Hi // P) * (Wi // P)
    cols = C * P * P
    ref = torch.nn.functional.unfold(f, P, stride=P).transpose(1, 2)             # [n, n_p, C*P*P], (c, ky, kx) order
    kidx = None
    if keep:
        n_keep = max(1, n_p // 3)
        kidx = torch.stack([torch.randperm(n_p, generator=g)[:n_keep] for _ in range(n)]).to(torch.int32)
        ref = torch.gather(ref, 1, kidx.long()[:, :, None].expand(-1, -1, cols))
    ref = ref.reshape(-1, cols).to(t)
    for src in (u8, f):
        obig = torch.full((ref.shape[0], cols + 16), -9.0, dtype=t, device=dev())
        L.patchify(src.to(dev()), obig[:, :cols], P, kidx.to(dev()) if keep else None)
        got = obig.cpu()
        assert torch.equal(got[:, :cols], ref), f'patchify {src.dtype}'
        assert (got[:, cols:] == -9.0).all()


def test_patchify_rejects_before_launch():
    """H % P, P % 8, n_keep > n_patches: A4R_EINVAL, nothing written (buffers sized so that a launch would stay in bounds)."""
    from adapter4rec_amd import _lib as L
    out = torch.full((64, 3 * 16 * 16), -3.0, device=dev())
    img = torch.zeros(1, 3, 40, 32, device=dev())
    img12 = torch.zeros(1, 3, 48, 48, device=dev())
    img32 = torch.zeros(1, 3, 32, 32, device=dev())
    keep = torch.arange(17, dtype=torch.int32, device=dev()).remainder(16)[None].contiguous()
    cases = {
        'H % P': lambda: L.patchify(img, out[:, :3 * 16 * 16], 16),
        'P % 8': lambda: L.patchify(img12, out[:, :3 * 12 * 12], 12),
        'n_keep > n_patches': lambda: L.patchify(img32, out[:, :3 * 8 * 8], 8, keep),
    }
    for what, call in cases.items():
        with pytest.raises(RuntimeError, match='invalid argument'):
            call()
        torch.cuda.synchronize()
        assert (out == -3.0).all(), f'{what}: output written'
