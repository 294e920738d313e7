"""tests/attn_ref.py and the cases of tests/test_attention_kernels_gpu.py, proved sound without a GPU.  For every case of attn_ref.CASES:
  (a) the written-out backward equals torch fp64 autograd of the plain additive-mask formula softmax(q k^T scale + (allowed ? 0 : mask_neg)) v to
      1e-12 relative -- wherever that formula IS the kernels' semantics in fp64: no row without an allowed key, or mask_neg = finfo.min (which
      swallows the score in fp64 as well), or -10000 (where such rows carry dO = 0);
  (b) max |scaled score| < 32 (the exact-mask precondition), and the key masks contain what the case claims;
  (c) the same formula in fp32 on the CPU is within the fp32 bounds; its maximum errors are printed ("fp32 CPU", the column the GPU file quotes), and
      for bf16 cases the bf16 model's worst (item, head) relative RMS error per tensor ("bf16 model");
  (d) the case's bounds (attn_ref.judge) REJECT every wrong reference that applies to it: key mask shifted by one key, last key tile dropped, causal
      boundary off by one, another site's keep mask in dK only, one head's K taken from its neighbour, and -- the persistent walk -- the rows of pair
      i + grid swapped with pair i.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import attn_ref as R

ALL = list(R.CASES)
WALK_CU = 8                       # the walk's cases at a pretended CU count of 8: 18 pairs, the same 2.5 pairs per workgroup


def _walk_case(S, drop):
    c = R.make_case(**R.walk_spec(WALK_CU, S, drop))
    c.ref = R.reference(c)
    c.fig = R.model_figures(c, c.ref)
    return c


def _autograd(c):
    """torch fp64 autograd of the plain additive-mask formula"""
    q, k, v = (t.clone().requires_grad_(True) for t in (c.q, c.k, c.v))
    s = (q @ k.transpose(-1, -2)) * c.scale
    if c.allowed is not None:
        s = s + torch.where(c.allowed, torch.zeros((), dtype=torch.float64), torch.full((), c.neg, dtype=torch.float64))
    p = torch.softmax(s, -1)
    if c.keepmul is not None:
        p = p * c.keepmul
    out = p @ v
    if c.lens is not None:
        out = out * c.valid[:, None, :, None]
    dq, dk, dv = torch.autograd.grad(out, [q, k, v], c.do)
    return SimpleNamespace(out=out.detach(), dq=dq, dk=dk, dv=dv)


@pytest.mark.parametrize('name', ALL)
def test_reference_equals_autograd(name):
    c = R.case(name)
    no_key_rows = bool((c.valid & ~c.any_key).any())
    if no_key_rows and c.neg == -1e9:
        # the additive formula in fp64 keeps s in such a row: it is NOT what fp32 computes (test_exact_mask_differs_from_additive_mask_in_fp64)
        return
    a = _autograd(c)
    for x in R.TENSORS:
        ref = getattr(c.ref, x)
        err = float((getattr(a, x) - ref).abs().max())
        assert err <= 1e-12 * max(1.0, float(ref.abs().max())), (name, x, err)


def test_exact_mask_differs_from_additive_mask_in_fp64():
    """Why -1e9 cases with a row without an allowed key are left out above: there fp64 `s - 1e9` keeps the score, fp32 does not."""
    c = R.case('long_f32_dh64_S33_causal' if R.CASES['long_f32_dh64_S33_causal']['neg'] == -1e9 else 'long_bf16_dh64_S33_causal')
    assert c.neg == -1e9 and bool((~c.any_key).any())
    a = _autograd(c)
    assert float((a.out - c.ref.out).abs().max()) > 1e-2
    q, k, v = c.q.float(), c.k.float(), c.v.float()
    s = (q @ k.transpose(-1, -2)) * c.scale + torch.where(c.allowed, torch.zeros(()), torch.full((), c.neg))
    out32 = torch.softmax(s, -1) @ v
    assert float((out32.double() - c.ref.out).abs().max()) < 1e-4


@pytest.mark.parametrize('name', ALL)
def test_case_preconditions(name):
    c = R.case(name)
    S = c.S
    assert c.smax < R.SMAX
    assert all(o * c.qkv.element_size() % 16 == 0 for o in c.off.values()) and c.ld > 3 * c.Hd and c.ldo > c.Hd
    assert sorted(c.off, key=c.off.get) == ['v', 'q', 'k']                          # a permuted block order
    assert (c.ld * c.qkv.element_size()) % 16 == 0 and (c.ldo * c.qkv.element_size()) % 16 == 0
    assert (c.n_items * c.nh) % 2 == 1 or c.family == 'long'                        # no multiple of the 4 / 2 waves (2 pairs) of a short workgroup
    if c.mask == 'all6':
        km = c.km
        assert c.n_items >= 6
        assert bool(km[0].all()) and not bool(km[2].any())                           # a full row, the all-PAD item
        assert int(km[5].sum()) == 1                                                 # a single key
        if S >= 4:
            L = int(km[1].sum())
            assert 0 < L < S and bool(km[1, :L].all())                               # ragged right
            assert not bool(km[3, :3].any()) and bool(km[3, 3:].all())               # left padding
            assert bool(km[4, 0]) and not bool(km[4, 1]) and not bool(km[4, 2]) and bool(km[4, 3])      # holes
        assert bool((~c.any_key).any())
        if c.causal and S >= 4:                                                      # left padding under causal: queries without any allowed key in a non-empty item
            assert bool((~c.any_key[3]).any()) and bool(c.any_key[3].any())
    if c.lens is not None:
        assert {1, 2, 15, 16, 17, 31, 32} == set(c.lens) and c.key_mask is None and int(c.offsets[-1]) == c.n_rows
    if c.drop > 0:
        frac = float((c.keepmul > 0).double().mean())
        assert abs(frac - (1 - c.drop)) < 4.0 * math.sqrt(c.drop * (1 - c.drop) / c.keepmul.numel()) + 1e-3, frac
    if c.neg > -1e9:                                                                 # -10000: rows without an allowed key carry no gradient
        assert float((c.do * (~c.any_key)[:, None, :, None]).abs().max()) == 0.0


def _fp32_eval(c):
    f = lambda t: None if t is None else t.float()
    out, lse, p, _ = R.forward_ref(f(c.q), f(c.k), f(c.v), c.allowed, c.scale, c.neg, f(c.keepmul))
    dq, dk, dv = R.backward_ref(f(c.q), f(c.k), f(c.v), f(c.do), p, c.scale, f(c.keepmul))
    return SimpleNamespace(out=out, dq=dq, dk=dk, dv=dv, lse=lse)


@pytest.mark.parametrize('name', ALL)
def test_fp32_and_bf16_columns(name):
    c = R.case(name)
    e = _fp32_eval(c)
    if c.lens is not None:
        for x in R.TENSORS:
            setattr(e, x, getattr(e, x) * c.valid[:, None, :, None])
    c32 = SimpleNamespace(**{**c.__dict__, 't': torch.float32})
    figs, fails = R.judge(c32, e, c.ref)
    lse_err = float(((e.lse.double() - c.ref.lse).abs() * (c.valid & c.any_key)[:, None, :]).max())      # (rows with an allowed key, as on the GPU)
    print(f'FP32 {name} ' + ' '.join(f'{x}={figs[x][0]:.1e}' for x in R.TENSORS) + f' lse={lse_err:.1e}')
    assert not fails, (name, fails)
    assert lse_err < 1e-4
    if c.t == torch.bfloat16:
        print(f'BF16MODEL {name} ' + ' '.join(f'{x}={c.fig[x][0]:.2e}/{c.fig[x][1]:.2e}' for x in R.TENSORS))
        m = R.bf16_model(c.q, c.k, c.v, c.do, c.ref.p, c.scale, c.keepmul, round_p=c.dh > 16, delta_from_out=c.family == 'long')
        _, fails = R.judge(c, dict(zip(R.TENSORS, m)), c.ref, {x: (math.inf, math.inf) for x in R.TENSORS})
        assert not fails, (name, fails)                                              # the model itself sits inside the elementwise bf16 bounds


# ------------------------------------------------------------------ (d) mutations
def _mut_key_shift(c):
    if c.km is None or c.lens is not None:
        return None
    return R.reference(c, allowed=R.allowed_of(torch.roll(c.km, 1, dims=1), c.S, c.causal))


def _mut_drop_last_tile(c):
    lo = (c.S - 1) // 16 * 16
    if lo == 0:
        return None
    a = c.allowed if c.allowed is not None else torch.ones(1, 1, c.S, c.S, dtype=torch.bool)
    return R.reference(c, allowed=a & (torch.arange(c.S) < lo))


def _mut_causal_off_by_one(c):
    if not c.causal:
        return None
    a = torch.tril(torch.ones(1, 1, c.S, c.S, dtype=torch.bool), diagonal=1)
    if c.km is not None:
        a = a & (c.km != 0)[:, None, None, :]
    if c.lens is not None:
        a = a & c.valid[:, None, None, :]
    return R.reference(c, allowed=a)


def _mut_other_site_in_dk(c):
    if c.drop <= 0:
        return None
    wrong = R.reference(c, keepmul=R.keep_multiplier(c, c.drop_site + 1))
    return SimpleNamespace(out=c.ref.out, dq=c.ref.dq, dk=wrong.dk, dv=c.ref.dv)


def _mut_neighbour_head_k(c):
    if c.nh < 2:
        return None
    k = c.k.clone()
    k[:, 1] = c.k[:, 0]                                                              # head 1 reads head 0's K
    return R.reference(c, k=k)


MUTATIONS = dict(key_shift=_mut_key_shift, drop_last_tile=_mut_drop_last_tile, causal_off_by_one=_mut_causal_off_by_one,
                 other_site_in_dk=_mut_other_site_in_dk, neighbour_head_k=_mut_neighbour_head_k)


def _changed(c, wrong):
    return any(not torch.equal(getattr(wrong, x), getattr(c.ref, x)) for x in R.TENSORS)


def _check_mutations(c):
    for m, fn in MUTATIONS.items():
        wrong = fn(c)
        if wrong is None:
            continue
        if not _changed(c, wrong):                                                   # (S = 1: a roll by one key is the identity)
            assert c.S <= 2 or (m == 'key_shift' and not c.any_key.any()), (c.name, m, 'the mutation changed nothing')
            continue
        _, fails = R.judge(c, wrong, c.ref, c.fig)
        assert fails, f'{c.name}: the bounds let the mutation {m} through'


@pytest.mark.parametrize('name', ALL)
def test_bounds_reject_mutations(name):
    _check_mutations(R.case(name))


@pytest.mark.parametrize('S', [197, 129])
@pytest.mark.parametrize('drop', [0.0, 0.25])
def test_walk_bounds_reject_pair_swap(S, drop):
    c = _walk_case(S, drop)
    n_pairs, grid = c.n_items * c.nh, WALK_CU
    assert 2 * grid < n_pairs < 3 * grid
    _check_mutations(c)
    _, fails = R.judge(c, c.ref, c.ref, c.fig)
    assert not fails
    perm = torch.arange(n_pairs)
    for i in range(n_pairs - grid):                                                  # what a workgroup computes from the wrong image set: pair i + grid's rows are pair i's
        if (i // grid) % 2 == 0:
            perm[i], perm[i + grid] = i + grid, i
    for only in R.TENSORS:                                                           # ... in each tensor alone
        wrong = {x: getattr(c.ref, x) for x in R.TENSORS}
        wrong[only] = wrong[only].reshape(n_pairs, c.S, c.dh)[perm].reshape(c.n_items, c.nh, c.S, c.dh)
        _, fails = R.judge(c, wrong, c.ref, c.fig)
        assert any(f.startswith(only) for f in fails), (only, fails)
    # one single swapped pair is enough
    wrong = {x: getattr(c.ref, x).clone() for x in R.TENSORS}
    flat = wrong['dq'].view(n_pairs, c.S, c.dh)
    flat[[1, 1 + grid]] = flat[[1 + grid, 1]]
    _, fails = R.judge(c, wrong, c.ref, c.fig)
    assert any(f.startswith('dq') for f in fails), fails


def test_every_mutation_has_a_family():
    """every mutation applies to many cases of the table, not to none"""
    C = list(R.CASES.values())
    n = dict(key_shift=sum(s.get('mask') == 'all6' and s['S'] > 2 for s in C), drop_last_tile=sum(s['S'] > 16 for s in C),
             causal_off_by_one=sum(bool(s.get('causal')) and s['S'] > 2 for s in C), other_site_in_dk=sum(s.get('drop', 0.0) > 0 and s['S'] > 2 for s in C),
             neighbour_head_k=sum(s['nh'] >= 2 and s['S'] > 2 for s in C))
    assert all(v >= 20 for v in n.values()), n


def test_case_list_covers_the_edges():
    """The shapes the GPU file is meant to reach are in the list (a guard against a quiet edit of the list)."""
    C = R.CASES
    short = [s for n, s in C.items() if n.startswith('short_')]
    for fam in ('scalar', 'mfma', 'wide'):
        mine = [s for s in short if R.kernel_family(s['dh']) == fam]
        assert {s['S'] for s in mine} == set(R.SHORT_S)
        assert {s['causal'] for s in mine} == {True, False}
        assert {s['neg'] for s in mine} == set(R.NEGS)
        assert {s['drop'] for s in mine} == {0.0, 0.25}
        assert {s['mask'] for s in mine} == {None, 'all6'} and {s['nh'] for s in mine} == {1, 3}
        assert {(s['neg'], s['mask']) for s in mine} >= {(n, 'all6') for n in R.NEGS}
    assert {(s['dt'], s['dh']) for s in short} == set(R.SHORT_COMBOS)
    for dt, dh in R.SHORT_COMBOS:
        mine = [s for s in short if (s['dt'], s['dh']) == (dt, dh)]
        assert {s['S'] for s in mine} == set(R.SHORT_S) and {s['drop'] for s in mine} == {0.0, 0.25} and {s['causal'] for s in mine} == {True, False}
    assert len(R.names('packed_')) == 4
    long_ = [s for n, s in C.items() if n.startswith('long_')]
    every_S = set(R.LONG_EDGES) | set(R.LONG_INNER)
    assert every_S == {1, 16, 17, 32, 33, 64, 65, 128, 129, 144, 145, 161, 193, 209, 224, 225, 241, 256}
    for S in every_S:
        assert {s['dt'] for s in long_ if s['S'] == S and s['dh'] in (32, 64)} == {'f32', 'bf16'}, S
    for S in R.LONG_EDGES:
        for dt, dh in R.LONG_COMBOS:
            modes = {(s.get('mask'), s.get('causal', False)) for s in long_ if (s['S'], s['dt'], s['dh']) == (S, dt, dh)}
            assert modes >= {(None, False), ('all6', False), ('all6', True)}, (S, dt, dh)
    for S in R.ONEPASS_S:
        assert {s.get('drop', 0.0) for s in long_ if (s['S'], s['dt'], s['dh'], s.get('mask')) == (S, 'bf16', 64, None)} == {0.0, 0.25}, S
    assert {s['S'] for s in long_ if s['dh'] == 128} == {17, 33, 65, 128}
    from adapter4rec_amd import _lib  # noqa: F401  (the package imports without a GPU)
    nkt = lambda S: 2 if S <= 32 else 4 if S <= 64 else 8 if S <= 128 else 14 if S <= 224 else 16          # nkt_for (a4r_attn_long.hip)
    for dt, dh in R.LONG_COMBOS:
        assert {nkt(s['S']) for s in long_ if (s['dt'], s['dh']) == (dt, dh) and s.get('drop', 0.0) > 0} == {2, 4, 8, 14, 16}
    assert {nkt(s['S']) for s in long_ if s['dh'] == 128 and s.get('drop', 0.0) > 0} == {2, 4, 8}
