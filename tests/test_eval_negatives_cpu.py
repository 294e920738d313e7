"""CPU side of the sampled evaluation's negatives drawn on the device (include/a4r_eval_negatives.h: a4r_eval_draw_negatives,
a4r_eval_rank_sampled): the C boundary of the two exports (header, the binding's table in adapter4rec_amd/_lib_eval_negatives.py, the built
library, refusals in front of the first HIP call), the properties of the draw rule on its restatement (tests/eval_neg_ref.py), the flags in both
parsers and their refusals, and eval_ranks / eval_model / write_eval_negatives on the stand-in library against the restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_neg_ref as NR
import lists_ref as LR
import sim_lib

NAMES = ['a4r_eval_draw_negatives', 'a4r_eval_rank_sampled']
HEADER = ('include', 'a4r_eval_negatives.h')
SEED = 0xA5A5F00D12345678


# ------------------------------------------------------------------ the C boundary, held as tests/test_user_lists_cpu.py holds its header
def neg_prototypes():
    import test_abi_cpu as ABI
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', ABI.header(HEADER)):
        params = []
        for a in args.split(','):
            words = re.sub(r'\bconst\b', ' ', a).replace('*', ' * ').split()
            params.append((words[0], '*' in words))
        assert name not in out, name
        out[name] = (ret, params)
    return out


def test_signature_table_matches_the_header_and_the_library():
    import test_abi_cpu as ABI
    from adapter4rec_amd import _lib as L
    protos = neg_prototypes()
    table = L.EVAL_NEGATIVES_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    assert not set(table) & (set(L.SIGNATURES) | set(L.SCORE_CE_BF16_SIGNATURES) | set(L.CANDIDATES_SIGNATURES) | set(L.USER_LISTS_SIGNATURES))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I, _U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert table['a4r_eval_draw_negatives'] == (_I, (_P,) * 6 + (_U,) + (_P,) * 2 + (_I,) * 3)
    assert table['a4r_eval_rank_sampled'] == (_I, (_P,) * 8 + (_U,) + (_P,) * 2 + (_I,) * 4)
    txt = ABI.header(HEADER)
    defines = dict(re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt))
    assert defines == {'A4R_EVAL_NEG_SITE': '7002'}
    assert L.EVAL_NEG_SITE == NR.EVAL_NEG_SITE == 7002 != L.SAMPLE_SITE and L.EVAL_NEG_MAX == L.LIST_MAX == NR.NEG_MAX and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    assert 'WITH replacement' in raw and 'pure function' in raw                   # the duplicate rule and the reproducibility are written down
    common = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'a4r_common.h')).read()
    assert '7002' in common                                                       # the site list names the new site
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert '#include "a4r_eval_negatives.h"' in a4r_h and '#include "a4r_user_lists.h"' in a4r_h
    assert a4r_h.index('#include "a4r_user_lists.h"') < a4r_h.index('#include "a4r_eval_negatives.h"')        # A4R_LIST_MAX comes first
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_eval_draw_negatives(*([None] * 6), 1.5, None, None, 4, 100, 10)


def test_wrappers_are_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_eval_negatives as B
    assert L.eval_draw_negatives is B.eval_draw_negatives and L.eval_rank_sampled is B.eval_rank_sampled
    assert L.EVAL_NEGATIVES_SIGNATURES is B.EVAL_NEGATIVES_SIGNATURES and L.EVAL_NEG_SITE == B.EVAL_NEG_SITE


def _bound(name):
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    restype, argtypes = L.EVAL_NEGATIVES_SIGNATURES[name]
    f = getattr(lib, name)
    f.argtypes, f.restype = argtypes, restype
    return f


def test_exports_refuse_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (nothing is enqueued, no GPU is needed): each pointer in turn NULL -- all but the stream and cdf,
    whose NULL means uniform sampling and is therefore only probed beside another bad argument -- then U < 1, N1 < 2, N outside 1 .. 4096, E not
    served, and prec / item_emb off a 16-byte boundary."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    draw, rank = _bound('a4r_eval_draw_negatives'), _bound('a4r_eval_rank_sampled')
    # draw: (stream, hist_ptr, hist_idx, target, user_key, cdf, seed, out_ids, err, U, N1, N)
    good = [None, p, p, p, p, p, 7, p, p, 16, 100, 10]
    probed = 0
    for i in (1, 2, 3, 4, 7, 8):
        a = list(good)
        a[i] = None
        assert draw(*a) == -1, i
        probed += 1
    for U, N1, N in ((0, 100, 10), (-1, 100, 10), (16, 1, 10), (16, 0, 10), (16, 100, 0), (16, 100, -1), (16, 100, 4097)):
        for cdf in (p, None):
            assert draw(None, p, p, p, p, cdf, 7, p, p, U, N1, N) == -1, (U, N1, N)
    assert draw(*([None] * 6), 0, None, None, 0, 0, 0) == -1
    # rank: (stream, prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, seed, rank, err, U, N1, E, N)
    good = [None, p, p, p, p, p, p, p, 7, p, p, 16, 100, 64, 10]
    for i in (1, 2, 3, 4, 5, 6, 9, 10):
        a = list(good)
        a[i] = None
        assert rank(*a) == -1, i
        probed += 1
    for U, N1, E, N in ((0, 100, 64, 10), (16, 1, 64, 10), (16, 100, 96, 10), (16, 100, 32, 10), (16, 100, 1024, 10), (16, 100, 0, 10),
                        (16, 100, 64, 0), (16, 100, 64, 4097), (16, 100, 512, -3)):
        for cdf in (p, None):
            assert rank(None, p, p, p, p, p, p, cdf, 7, p, p, U, N1, E, N) == -1, (U, N1, E, N)
    for which in (1, 2):
        a = list(good)
        a[which] = p + 4
        assert rank(*a) == -1, which
    assert rank(*([None] * 8), 0, None, None, 0, 0, 0, 0) == -1
    assert probed == 6 + 8


def test_wrappers_refuse_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, U, E, n = 9, 4, 64, 5
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good_d = dict(hist_ptr=i32(U + 1), hist_idx=i32(3), target=i32(U), user_key=i32(U), cdf=None, seed=1, n1=N1, out_ids=i32(U, n), err=i32(1))
    good_r = dict(prec=torch.zeros(U, E), item_emb=torch.zeros(N1, E), target=i32(U), hist_ptr=i32(U + 1), hist_idx=i32(3), user_key=i32(U), cdf=None,
                  seed=1, n=n, rank=i32(U), err=i32(1))
    draw = lambda **kw: L.eval_draw_negatives(**dict(good_d, **kw))
    rank = lambda **kw: L.eval_rank_sampled(**dict(good_r, **kw))
    both = [(dict(hist_ptr=i32(U)), 'hist_ptr'), (dict(hist_ptr=i32(U + 1).long()), 'hist_ptr'), (dict(hist_idx=torch.zeros(3)), 'hist_idx'),
            (dict(target=i32(U).long()), 'target'), (dict(user_key=i32(U + 1)), 'user_key'), (dict(user_key=i32(U).long()), 'user_key'),
            (dict(err=i32(2)), 'err'), (dict(err=torch.zeros(1)), 'err'), (dict(cdf=torch.zeros(N1, dtype=torch.int32)), 'cdf'),
            (dict(cdf=torch.zeros(N1 + 1, dtype=torch.int64)), 'cdf'), (dict(seed=-1), 'seed'), (dict(seed=2 ** 64), 'seed')]
    for kw, msg in both + [(dict(out_ids=i32(U, L.EVAL_NEG_MAX + 1)), 'n = 4097'), (dict(out_ids=i32(U + 1, n)), 'out_ids'), (dict(out_ids=i32(U * n)), 'out_ids'),
                           (dict(out_ids=i32(U, n).long()), 'out_ids'), (dict(n1=1), 'N1 = 1')]:
        with pytest.raises(ValueError, match=msg):
            draw(**kw)
    for kw, msg in both + [(dict(n=0), 'n = 0'), (dict(n=4097), 'n = 4097'), (dict(prec=torch.zeros(U, E, dtype=torch.float64)), 'prec'),
                           (dict(item_emb=torch.zeros(N1, 128)), 'expected'), (dict(prec=torch.zeros(U, 96), item_emb=torch.zeros(N1, 96)), 'E = 96'),
                           (dict(item_emb=torch.zeros(1, E)), 'N1 = 1'), (dict(prec=torch.zeros(U + 1, E)), 'rows'), (dict(rank=i32(U + 1)), 'rank'),
                           (dict(rank=torch.zeros(U)), 'rank')]:
        with pytest.raises(ValueError, match=msg):
            rank(**kw)


# ------------------------------------------------------------------ the rule itself
def _chi2_limit(dof, z=3.72):
    """the 1 - 1e-4 quantile of chi-square by Wilson-Hilferty (the draws are fixed by the seed: the test cannot flake, the limit only has to be one
    that a wrong distribution misses)"""
    return dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3


def _many_draws(hist, target, N1, cdf, total=200000):
    n = 4000
    return np.concatenate([NR.user_draws(hist, target, 1000 + k, N1, n, SEED, cdf)[0] for k in range(total // n)])


def test_draws_avoid_the_exclusion_set_and_follow_the_weights():
    """never a member of D, the pad row or a zero-count item; chi-square of 200 000 draws against the weights renormalised over the complement
    of D, for both samplings"""
    rng = np.random.default_rng(21)
    N1 = 40
    hist = [3, 17, 17, 0, -4, 39, N1, N1 + 7]
    target = 22
    D = NR.exclusion_set(hist, target, N1)
    assert D == [3, 17, 22, 39]
    ids = _many_draws(hist, target, N1, None)
    assert ids.min() >= 1 and ids.max() < N1 and not set(ids.tolist()) & set(D)
    obs = np.bincount(ids, minlength=N1)[[i for i in range(1, N1) if i not in D]]
    exp = ids.size / obs.size
    chi = float(((obs - exp) ** 2 / exp).sum())
    print(f'uniform: chi-square {chi:.1f} at {obs.size - 1} dof')
    assert obs.size == 35 and chi < _chi2_limit(obs.size - 1)
    cnt = rng.integers(1, 30, size=N1 - 1)
    cnt[[4, 9, 10, 30, 38]] = 0                                                   # items 5, 10, 11, 31, 39: never drawn (39 is in D as well)
    cdf = NR.make_cdf(cnt, N1)
    ids = _many_draws(hist, target, N1, cdf)
    live = [i for i in range(1, N1) if i not in D and cnt[i - 1] > 0]
    assert set(ids.tolist()) <= set(live)
    obs = np.bincount(ids, minlength=N1)[live]
    w = cnt[[i - 1 for i in live]].astype(np.float64)
    exp = ids.size * w / w.sum()
    chi = float(((obs - exp) ** 2 / exp).sum())
    print(f'weighted: chi-square {chi:.1f} at {len(live) - 1} dof')
    assert chi < _chi2_limit(len(live) - 1) and exp.min() > 5


def test_draws_are_a_function_of_the_user_alone():
    """the draws of a user do not change with the batch around it, its order or its size; they change with the seed, the key and D"""
    rng = np.random.default_rng(22)
    N1, n, U = 500, 50, 12
    hists = [rng.integers(0, N1, size=int(rng.integers(0, 40))) for _ in range(U)]
    target = rng.integers(1, N1, size=U)
    keys = rng.integers(0, 2 ** 31, size=U)
    cdf = NR.make_cdf(rng.integers(0, 9, size=N1 - 1), N1)
    for c in (None, cdf):
        full, err = NR.draw_negatives(hists, target, keys, N1, n, SEED, c)
        assert err == 0
        perm = rng.permutation(U)
        got, _ = NR.draw_negatives([hists[i] for i in perm], target[perm], keys[perm], N1, n, SEED, c)
        np.testing.assert_array_equal(got, full[perm])
        np.testing.assert_array_equal(NR.draw_negatives(hists[5:6], target[5:6], keys[5:6], N1, n, SEED, c)[0], full[5:6])
        np.testing.assert_array_equal(NR.draw_negatives(hists[2:9], target[2:9], keys[2:9], N1, n, SEED, c)[0], full[2:9])
        np.testing.assert_array_equal(NR.user_draws(hists[0], target[0], keys[0], N1, 20, SEED, c)[0], full[0, :20])       # draw j does not depend on N
        assert (NR.user_draws(hists[0], target[0], keys[0], N1, n, SEED + 1, c)[0] != full[0]).mean() > 0.8
        assert (NR.user_draws(hists[0], target[0], keys[0] ^ 1, N1, n, SEED, c)[0] != full[0]).mean() > 0.8
    assert NR.user_draws([], 1, 0, 3, 4, SEED)[0].tolist() == [2, 2, 2, 2]           # keys 0 and 2^31 - 1, negative keys as their 32 bits
    assert (NR.user_draws([], 1, -1, 900, 30, SEED)[0] == NR.user_draws([], 1, 2 ** 32 - 1 - 2 ** 32, 900, 30, SEED)[0]).all()


def test_no_candidate_gives_zeros_and_is_counted():
    N1 = 6
    everything = [1, 2, 3, 4, 5]
    ids, m = NR.user_draws(everything, 0, 3, N1, 7, SEED)
    assert m == 0 and (ids == 0).all()
    ids, m = NR.user_draws([1, 2, 3, 4], 5, 3, N1, 7, SEED)                          # the target takes the last candidate
    assert m == 0 and (ids == 0).all()
    ids, m = NR.user_draws([1, 2, 4, 5, 5, 0], 9, 3, N1, 7, SEED)
    assert m == 1 and (ids == 3).all()
    cdf = NR.make_cdf([4, 0, 0, 2, 0], N1)                                           # only items 1 and 4 can be drawn
    assert NR.user_draws([1, 4], 2, 3, N1, 7, SEED, cdf)[1] == 0
    ids, m = NR.user_draws([4], 2, 3, N1, 7, SEED, cdf)
    assert m == 4 and (ids == 1).all()
    out, err = NR.draw_negatives([everything, [1], [1, 2, 3, 4], []], [0, 2, 5, 1], [0, 1, 2, 3], N1, 3, SEED)
    assert err == 2 and (out[[0, 2]] == 0).all() and (out[[1, 3]] > 0).all()
    s = np.arange(24, dtype=np.float64).reshape(4, 6)
    r, err = NR.rank_sampled_reference(s, [everything, [1], [1, 2, 3, 4], []], [0, 2, 5, 1], [0, 1, 2, 3], 3, SEED)
    assert err == 2 and r[0] == r[2] == 1 and r[3] > 1


def test_counts_of_2_to_the_40_take_the_64_bit_path():
    rng = np.random.default_rng(23)
    N1 = 300
    cnt = [int(c) for c in rng.integers(0, 3, size=N1 - 1)]
    heavy = [20, 150, 151, 298]
    for i in heavy:
        cnt[i - 1] = 2 ** 40
    cdf = NR.make_cdf(cnt, N1)
    assert cdf[-1] > 2 ** 42
    ids, m = NR.user_draws([150, 7, 8], 299, 5, N1, 3000, SEED, cdf)
    assert m > 2 ** 41 and set(np.unique(ids).tolist()) <= set(range(1, N1)) - {150, 7, 8, 299}
    share = np.bincount(ids, minlength=N1)[[20, 151, 298]] / ids.size
    assert (np.abs(share - 1 / 3) < 0.03).all()                                   # the three heavy items outside D share the draws
    assert all(cnt[i - 1] > 0 for i in np.unique(ids))


# ------------------------------------------------------------------ the flags
def test_both_parsers_take_the_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert a.eval_negatives == 0 and a.eval_neg_sampling == 'uniform' and a.eval_neg_seed == 20240607 and a.eval_negatives_out is None
        a = parse(['--mode', 'test', '--eval_negatives', '100', '--eval_neg_sampling', 'pop', '--eval_neg_seed', '9', '--eval_negatives_out', 'neg.tsv'])
        assert (a.eval_negatives, a.eval_neg_sampling, a.eval_neg_seed, a.eval_negatives_out) == (100, 'pop', 9, 'neg.tsv')
        with pytest.raises(SystemExit):
            parse(['--eval_neg_sampling', 'zipf'])


def test_flags_are_refused_where_they_do_not_apply():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    for main in (run.main, run_adapter.main):
        with pytest.raises(ValueError, match='--mode recommend'):
            main(['--mode', 'recommend', '--eval_negatives', '100'])
        with pytest.raises(ValueError, match='cannot be combined'):
            main(['--mode', 'test', '--eval_negatives', '100', '--candidate_lists', 'l.tsv'])
        with pytest.raises(ValueError, match='cannot be combined'):
            main(['--mode', 'test', '--eval_negatives', '100', '--candidate_items', 'c.txt'])
        with pytest.raises(ValueError, match='--eval_negatives_out'):
            main(['--mode', 'train', '--eval_negatives', '100', '--eval_negatives_out', 'n.tsv'])
        with pytest.raises(ValueError, match='--eval_negatives_out'):
            main(['--mode', 'test', '--eval_negatives_out', 'n.tsv'])
        for n in ('4097', '-1'):
            with pytest.raises(ValueError, match='outside 1 .. 4096'):
                main(['--mode', 'test', '--eval_negatives', n])
        with pytest.raises(ValueError, match='--eval_neg_seed'):
            main(['--mode', 'test', '--eval_negatives', '10', '--eval_neg_seed', '-5'])


# ------------------------------------------------------------------ the Python API on the stand-in library
CALLS = []


def sim_eval_rank_sampled(prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, seed, n, rank, err):
    assert user_key.dtype == torch.int32 and user_key.numel() == prec.shape[0] and err.dtype == torch.int32 and err.numel() == 1
    assert cdf is None or (cdf.dtype == torch.int64 and cdf.numel() == item_emb.shape[0] and int(cdf[0]) == 0)
    CALLS.append((prec.detach().clone(), user_key.clone()))
    return NR.sim_eval_rank_sampled(prec, item_emb, target, hist_ptr, hist_idx, user_key, cdf, seed, n, rank, err)


def _refuse(*a, **k):
    raise AssertionError('another entry called under eval_negatives / a sampled call without it')


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', sim_eval_rank_sampled, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_draw_negatives', NR.sim_eval_draw_negatives, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', LR.sim_eval_rank_lists, raising=False)
    CALLS.clear()


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


@pytest.mark.parametrize('sampling', ['uniform', 'pop'])
def test_eval_model_against_the_restatement(simulated, monkeypatch, tmp_path, sampling):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import (EvalNegatives, eval_model, eval_ranks, item_counts, read_candidate_lists,
                                                    write_eval_negatives)
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(24)
    U, N1, n = len(eval_seq), item_num + 1, 30
    target = np.array([eval_seq[u][-1] for u in range(U)])
    hlists = [hist[u].numpy() for u in range(U)]
    counts = None
    if sampling == 'pop':
        counts = item_counts({u: eval_seq[u][:-1] for u in range(U)}, item_num)
        assert counts.shape == (N1,) and counts[0] == 0 and counts.sum() == sum(len(eval_seq[u]) - 1 for u in range(U))
        keep = set(eval_seq[3])                                                   # only user 3's own items can be drawn: user 3 is left with none
        counts = np.array([max(c, 1) if i in keep else 0 for i, c in enumerate(counts)], np.int64)
    spec = EvalNegatives(n, seed=SEED, counts=counts)
    cdf = None if counts is None else NR.make_cdf(counts[1:], N1)
    for name in ('eval_rank', 'eval_rank_cand', 'eval_rank_lists'):
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)               # under eval_negatives, no other entry is called
    ranks = eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), eval_negatives=spec).numpy()
    prec = torch.cat([c[0] for c in CALLS]).double().numpy()
    np.testing.assert_array_equal(torch.cat([c[1] for c in CALLS]).numpy(), np.arange(U))      # the key is the global user id
    s64 = prec @ emb.double().numpy().T
    want, want_err = NR.rank_sampled_reference(s64, hlists, target, np.arange(U), n, SEED, cdf)
    np.testing.assert_array_equal(ranks, want)
    assert int(spec.last_err.item()) == want_err and (ranks > 1).any()
    ms = np.array([NR.user_draws(hlists[u], target[u], u, N1, 1, SEED, cdf)[1] for u in range(U)])
    valid = ms >= 1
    assert want_err == int((~valid).sum()) and (want_err > 0) == (sampling == 'pop')
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', eval_negatives=spec)
    hit, ndcg, k = LR.hit_ndcg_means(want, valid)
    assert abs(hr - hit) < 1e-7 and k == int(valid.sum())
    line = [l for l in log.lines if 'test_results' in l][0]
    np.testing.assert_allclose([float(x) for x in line.split()[1:]], [hit * 100, ndcg * 100], atol=1e-4)
    assert [l for l in log.lines if l.startswith('test_eval_negatives')] == [f'test_eval_negatives   {k} of {U} users']
    # the user batch does not enter: the same figures at 7 users a call (and a run of 24 users takes 4 calls)
    CALLS.clear()
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '7')
    log7 = _Log()
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, log7, 'test', 'cpu', eval_negatives=spec) == hr
    assert len(CALLS) == 4 and [l for l in log7.lines if 'test_results' in l] == [line]
    monkeypatch.delenv('A4R_EVAL_USER_BATCH')
    # the written draws, read back as candidate lists, give the same figures through the list entry
    user_names = [f'U{u}' for u in range(U)]
    item_names = [None] + [f'N{i}' for i in range(1, N1)]
    path = str(tmp_path / 'neg.tsv')
    assert write_eval_negatives(spec, hist, eval_seq, N1, args, user_names, item_names, path, torch.device('cpu')) == k
    lists = read_candidate_lists(path, user_names, item_names)
    ids, _ = NR.draw_negatives(hlists, target, np.arange(U), N1, n, SEED, cdf)
    assert lists == {u: ids[u].tolist() for u in range(U) if valid[u]}
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', LR.sim_eval_rank_lists)
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', _refuse)
    log2 = _Log()
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, log2, 'test', 'cpu', candidate_lists=lists) == hr
    assert [l for l in log2.lines if 'test_results' in l] == [line]
    # refusals
    for kw in (dict(candidates=np.ones(N1, bool)), dict(candidate_lists=lists)):
        with pytest.raises(ValueError, match='cannot be combined'):
            eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', eval_negatives=spec, **kw)
    for bad in (dict(n=0), dict(n=4097), dict(n=5, seed=-1), dict(n=5, counts=np.array([0, -1, 2])), dict(n=5, counts=np.array([0.5, 1.0]))):
        with pytest.raises(ValueError, match='eval_negatives'):
            EvalNegatives(**bad)
    with pytest.raises(ValueError, match='counts for a table'):
        eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), eval_negatives=EvalNegatives(5, counts=np.ones(N1 + 3, np.int64)))


def test_without_the_spec_the_sampled_wrapper_is_never_called(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import eval_model
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(20)
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', _refuse)
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu')
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', eval_negatives=None) == hr
    assert not any('users' in l for l in log.lines)


# ------------------------------------------------------------------ the text entry point
def test_text_runner_with_eval_negatives(tmp_path, monkeypatch):
    """train one epoch through run.py with --eval_negatives (the per-epoch evaluation draws), then --mode test --eval_negatives
    --eval_neg_sampling pop --eval_negatives_out from its checkpoint: both splits ranked among drawn negatives, `k of n users` beside each metrics
    line, the file written for every user of the test split -- and --mode test --candidate_lists on that file alone gives the test split's line
    again."""
    import glob
    import json
    import logging
    import socket
    import torch.distributed as dist
    import test_text_run as TR
    import test_topk_cpu as TC
    from adapter4rec_amd import run
    TC._simulated(monkeypatch)
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', sim_eval_rank_sampled, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_draw_negatives', NR.sim_eval_draw_negatives, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', LR.sim_eval_rank_lists, raising=False)
    root = str(tmp_path)
    data = TR.write_toy(root)
    cp = os.path.join(root, 'pretrained_models', 'bert', 'bert_tiny', 'config.json')
    c = json.load(open(cp))
    c.update(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)          # (the simulated library has no dropout)
    json.dump(c, open(cp, 'w'))
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data, '--dataset', 'toy', '--behaviors', 'behaviors.tsv', '--news', 'news.tsv', '--bert_model_load', 'bert_tiny',
              '--freeze_paras_before', '0', '--adapter_type', 'houslby', '--adding_adapter_to', 'all', '--fine_tune_to', 'None',
              '--pretrained_model_name', 'None', '--embedding_dim', '64', '--batch_size', '16', '--num_workers', '1', '--logging_num', '3',
              '--testing_num', '1', '--max_seq_len', '20', '--min_seq_len', '5', '--lr', '1e-3', '--adapter_bert_lr', '1e-3',
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'negs']
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())

    def main(argv):
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        for k, v in dict(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='1', RANK='0', LOCAL_RANK='0').items():
            monkeypatch.setenv(k, v)
        del seen[:]
        logging.getLogger('Log_file').addHandler(Keep())
        try:
            run.main(common + argv)
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
            for name in ('Log_file', 'Log_screen'):
                lg = logging.getLogger(name)
                for h in list(lg.handlers):
                    lg.removeHandler(h)
                    h.close()
        return list(seen)
    monkeypatch.setattr(sim_lib, 'eval_rank', _refuse)                            # with the flag no whole-table rank is taken
    CALLS.clear()
    lines = main(['--mode', 'train', '--epoch', '1', '--eval_negatives', '20'])
    assert any(l.startswith('eval negatives: 20 per user, uniform sampling') for l in lines)
    assert [l.split()[0] for l in lines if '_eval_negatives ' in l] == ['valid_eval_negatives', 'test_eval_negatives'] and len(CALLS) >= 2
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    out = os.path.join(root, 'neg.tsv')
    test = ['--mode', 'test', '--load_ckpt_name', 'epoch-1.pt']
    lines = main(test + ['--eval_negatives', '20', '--eval_neg_sampling', 'pop', '--eval_neg_seed', '11', '--eval_negatives_out', out])
    assert any(l.startswith('eval negatives: 20 per user, pop sampling, seed 11') for l in lines)
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    user_names, _ = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert [r[0] for r in rows] == list(user_names) and all(len(r[1].split(' ')) == 20 for r in rows)
    for split in ('valid', 'test'):
        assert [l for l in lines if l.startswith(split + '_eval_negatives')] == ['%s_eval_negatives   %d of %d users' % (split, len(user_names), len(user_names))]
    want = [l for l in lines if l.startswith('test_results')]
    assert len(want) == 1
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', _refuse)
    lines = main(test + ['--candidate_lists', out])
    assert [l for l in lines if l.startswith('test_results')] == want


# ------------------------------------------------------------------ the image entry point (--item_tower id: the kernel sees only prec and the table)
def test_id_runner_with_eval_negatives(tmp_path, monkeypatch):
    """run_adapter.py --item_tower id: one epoch with --eval_negatives (the per-epoch evaluation), then --mode test with popularity sampling and
    --eval_negatives_out, whose file given to --candidate_lists alone repeats the test split's line"""
    import logging
    import socket
    import torch.distributed as dist
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    from adapter4rec_amd.cv import run_adapter as RA
    for name in ('id_index', 'id_grad_sum', 'id_index_ws_ints'):
        monkeypatch.setattr(sim_lib, name, getattr(IC, name), raising=False)
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', sim_eval_rank_sampled, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_draw_negatives', NR.sim_eval_draw_negatives, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', LR.sim_eval_rank_lists, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank', _refuse, raising=False)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())

    def main(argv):
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        for k, v in dict(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='1', RANK='0', LOCAL_RANK='0').items():
            monkeypatch.setenv(k, v)
        del seen[:]
        logging.getLogger('Log_file').addHandler(Keep())
        try:
            RA.main(common + argv)
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
            for name in ('Log_file', 'Log_screen'):
                lg = logging.getLogger(name)
                for h in list(lg.handlers):
                    lg.removeHandler(h)
                    h.close()
        return list(seen)
    CALLS.clear()
    lines = main(['--epoch', '1', '--eval_negatives', '15'])
    assert [l.split()[0] for l in lines if '_eval_negatives ' in l] == ['valid_eval_negatives', 'test_eval_negatives'] and len(CALLS) >= 2
    out = os.path.join(root, 'neg.tsv')
    test = ['--mode', 'test', '--load_ckpt_name', 'epoch-1.pt']
    lines = main(test + ['--eval_negatives', '15', '--eval_neg_sampling', 'pop', '--eval_negatives_out', out])
    assert any(l.startswith('eval negatives: 15 per user, pop sampling') for l in lines)
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert len(rows) == CR.N_USERS_T and all(len(r[1].split(' ')) == 15 for r in rows)
    want = [l for l in lines if l.startswith('test_results')]
    assert len(want) == 1 and [l for l in lines if l.startswith('test_eval_negatives')] == ['test_eval_negatives   %d of %d users' % (len(rows), len(rows))]
    monkeypatch.setattr(sim_lib, 'eval_rank_sampled', _refuse)
    lines = main(test + ['--candidate_lists', out])
    assert [l for l in lines if l.startswith('test_results')] == want
