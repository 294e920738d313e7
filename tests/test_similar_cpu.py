"""CPU side of the similar-item queries (include/a4r_similar.h: a4r_row_inv_norms, a4r_topk_similar): the C boundary of the exports (header, the
binding's table in adapter4rec_amd/_lib_similar.py, the built library, refusals in front of the first HIP call), the properties of the rule on its
restatement (tests/similar_ref.py), the flags in both parsers and their refusals, and similar_items / write_similar_items / both runners on the
stand-in library."""
import ctypes
import glob
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

import similar_ref as SR
import sim_lib

NAMES = ['a4r_row_inv_norms', 'a4r_topk_similar']
HEADER = ('include', 'a4r_similar.h')


# ------------------------------------------------------------------ the C boundary, held as tests/test_mmr_cpu.py holds its header
def similar_prototypes():
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
    protos = similar_prototypes()
    table = L.SIMILAR_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    others = [t for m, (t, _) in L.SATELLITES.items() if m != '_lib_similar']
    assert '_lib_similar' in L.SATELLITES and len(others) == len(L.SATELLITES) - 1
    assert not set(table) & set(L.SIGNATURES).union(*(set(getattr(L, t)) for t in others))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert table['a4r_row_inv_norms'] == (_I, (_P, _P, _P, _I, _I))
    assert table['a4r_topk_similar'] == (_I, (_P,) * 5 + (_F,) + (_P,) * 3 + (_I,) * 4)
    txt = ABI.header(HEADER)
    assert not re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt) and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    for phrase in ('the query itself', 'ties to the smaller id', 'no table row is read', 'does not depend on the grid', 'before any HIP call'):
        assert phrase in raw, phrase                                               # the rule is written down
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert a4r_h.count('#include "a4r_similar.h"') == 1
    assert a4r_h.index('#include "a4r_diversify.h"') < a4r_h.index('#include "a4r_similar.h"')
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_topk_similar(*([None] * 5), 'floor', None, None, None, 1, 2, 64, 1)
    mk = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'Makefile')).read()
    assert mk.count('../../include/a4r_similar.h') == 3                            # the header in the three dependency lists
    src = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'a4r_topk.hip')).read()
    assert 'similar_partial_kernel' in src and 'extern "C" int a4r_topk_similar' in src      # a sibling of topk_partial_kernel, in its file


def test_wrappers_are_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_similar as B
    assert L.topk_similar is B.topk_similar and L.row_inv_norms is B.row_inv_norms and L.SIMILAR_SIGNATURES is B.SIMILAR_SIGNATURES


def test_exports_refuse_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (nothing is enqueued, no GPU is needed): each required pointer in turn NULL (inv_norm and cand may
    be NULL: the dot metric, no restriction -- every probe runs with and without them), E not served, K outside 1 .. 256, Q < 1, N1 < 2, item_emb
    off a 16-byte boundary, ws off an 8-byte boundary, min_sim NaN; the same for a4r_row_inv_norms."""
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    f, g = lib.a4r_topk_similar, lib.a4r_row_inv_norms
    f.restype, f.argtypes = L.SIMILAR_SIGNATURES['a4r_topk_similar']
    g.restype, g.argtypes = L.SIMILAR_SIGNATURES['a4r_row_inv_norms']
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    ninf, nan = -float('inf'), float('nan')
    # (stream, item_emb, inv_norm, query, cand, min_sim, ids, scores, ws, Q, N1, E, K)
    good = [None, p, p, p, p, ninf, p, p, p, 4, 100, 64, 10]
    optional = [(p, p), (None, p), (p, None), (None, None)]
    probed = 0

    def refused(i, v):
        for inv, cand in optional:
            a = list(good)
            a[2], a[4] = inv, cand
            a[i] = v
            assert f(*a) == -1, (i, v, inv, cand)
        return 1
    for i in (1, 3, 6, 7, 8):
        probed += refused(i, None)
    bad = [(11, 0), (11, 32), (11, 96), (11, 1024), (11, -64), (12, 0), (12, -1), (12, 257), (9, 0), (9, -1), (10, 1), (10, 0), (10, -5), (5, nan),
           (1, p + 4), (1, p + 8), (1, p + 12), (8, p + 4), (8, p + 1)]
    for i, v in bad:
        probed += refused(i, v)
    assert f(None, None, None, None, None, 0.0, None, None, None, 0, 0, 0, 0) == -1
    assert probed == 5 + len(bad)
    # (stream, table, inv, N1, E)
    for a in ([None, None, p, 10, 64], [None, p, None, 10, 64], [None, p, p, 0, 64], [None, p, p, -1, 64], [None, p, p, 10, 0], [None, p, p, 10, 96],
              [None, p, p, 10, 1024], [None, p + 4, p, 10, 64], [None, p + 8, p, 10, 64], [None, None, None, 0, 0]):
        assert g(*a) == -1, a


def test_wrappers_refuse_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, Q, E, k = 9, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(item_emb=torch.zeros(N1, E), inv_norm=torch.zeros(N1), query=i32(Q), cand=torch.ones(N1, dtype=torch.uint8), min_sim=None, k=k,
                ids=i32(Q, k), scores=torch.zeros(Q, k))
    call = lambda **kw: L.topk_similar(**dict(good, **kw))
    wide = torch.zeros(N1, 2 * E)[:, :E]
    off = torch.zeros(N1 * E + 1)[1:].view(N1, E)
    assert off.data_ptr() % 16 == 4 and not wide.is_contiguous()
    for kw, msg in [(dict(item_emb=torch.zeros(N1, E, dtype=torch.float64)), 'item_emb'), (dict(item_emb=wide), 'item_emb'), (dict(item_emb=off), 'aligned'),
                    (dict(item_emb=torch.zeros(N1, 96)), 'E = 96'), (dict(item_emb=torch.zeros(1, E), inv_norm=None, cand=None), 'N1 = 1'),
                    (dict(item_emb=torch.zeros(N1 * E)), 'expected'), (dict(query=i32(Q).long()), 'query'), (dict(query=i32(Q, 1)), 'query'),
                    (dict(query=i32(2 * Q)[::2]), 'query'), (dict(query=i32(0), ids=i32(0, k), scores=torch.zeros(0, k)), 'Q = 0'),
                    (dict(inv_norm=torch.zeros(N1 + 1)), 'inv_norm'), (dict(inv_norm=torch.zeros(N1, dtype=torch.float64)), 'inv_norm'),
                    (dict(inv_norm=torch.zeros(N1, 1)), 'inv_norm'), (dict(cand=torch.ones(N1 + 1, dtype=torch.uint8)), 'cand'),
                    (dict(cand=torch.ones(N1, dtype=torch.int32)), 'cand'), (dict(cand=torch.ones(2 * N1, dtype=torch.uint8)[::2]), 'cand'),
                    (dict(k=0), 'k = 0'), (dict(k=257), 'k = 257'), (dict(min_sim=float('nan')), 'min_sim'),
                    (dict(ids=i32(Q, k + 1)), 'ids and scores'), (dict(ids=i32(Q, k).long()), 'ids'), (dict(scores=torch.zeros(Q + 1, k)), 'ids and scores'),
                    (dict(scores=torch.zeros(Q, k, dtype=torch.float64)), 'scores')]:
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    for kw, msg in [(dict(table=torch.zeros(N1, E, dtype=torch.float64)), 'item_emb'), (dict(table=wide), 'item_emb'), (dict(table=off), 'aligned'),
                    (dict(table=torch.zeros(N1, 96)), 'E = 96'), (dict(table=torch.zeros(0, E)), 'N1 = 0'), (dict(table=torch.zeros(E)), 'expected'),
                    (dict(table=torch.zeros(N1, E), out=torch.zeros(N1 + 1)), 'out'), (dict(table=torch.zeros(N1, E), out=torch.zeros(N1, dtype=torch.float64)), 'out')]:
        with pytest.raises(ValueError, match=msg):
            L.row_inv_norms(**kw)
    with pytest.raises(RuntimeError, match='device tensors'):
        monkeypatch.undo()
        L.topk_similar(**good)                                                     # host tensors never reach a kernel
    with pytest.raises(RuntimeError, match='device tensors'):
        L.row_inv_norms(torch.zeros(N1, E))


# ------------------------------------------------------------------ the rule itself, on the restatement
def _brute(t, q, k, metric, cand=None, floor=None):
    """one query, from the definition, pair by pair in Python floats"""
    N1 = t.shape[0]
    ss = [float(np.dot(t[i].astype(np.float64), t[i].astype(np.float64))) for i in range(N1)]
    inv = [1.0 / np.sqrt(s) if (s > 0 and np.isfinite(s)) else 0.0 for s in ss]
    if not 1 <= q < N1 or (metric == 'cos' and inv[q] == 0):
        return [0] * k, [-np.inf] * k
    rows = []
    for i in range(1, N1):
        if i == q or (cand is not None and not cand[i]) or (metric == 'cos' and inv[i] == 0):
            continue
        s = float(np.dot(t[q].astype(np.float64), t[i].astype(np.float64)))
        if metric == 'cos':
            s = s * (inv[q] * inv[i])
        if np.isnan(s) or (floor is not None and not s >= floor):
            continue
        rows.append((-s, i))
    rows.sort()
    ids = [i for _, i in rows[:k]] + [0] * (k - min(k, len(rows)))
    sc = [-s + 0.0 for s, _ in rows[:k]] + [-np.inf] * (k - min(k, len(rows)))
    return ids, sc


def test_restatement_against_the_definition():
    rng = np.random.default_rng(2)
    N1, E = 40, 64
    t = SR.exact_cosine_table(rng, N1, E)
    t[7], t[9], t[30] = t[3], t[3] * 2, 0
    t[31, 5] = np.nan
    cand = rng.random(N1) < 0.6
    query = [3, 7, 9, 30, 31, 0, -2, N1, 12, 12]
    for metric in ('cos', 'dot'):
        tab = t if metric == 'cos' else np.nan_to_num(t)
        for kw in (dict(), dict(cand=cand), dict(min_sim=0.125), dict(cand=cand, min_sim=-0.25)):
            ids, sc = SR.similar_reference(torch.from_numpy(tab), query, 6, metric, **kw)
            for r, q in enumerate(query):
                bi, bs = _brute(tab, q, 6, metric, kw.get('cand'), kw.get('min_sim'))
                assert ids[r].tolist() == bi and sc[r].tolist() == bs, (metric, kw.keys(), q)
    # self never listed; duplicates list each other first at score 1, by id; dead rows are no one's neighbour and have none (cos)
    ids, sc = SR.similar_reference(torch.from_numpy(t), query, 6, 'cos')
    assert ids[0, :2].tolist() == [7, 9] and ids[1, :2].tolist() == [3, 9] and ids[2, :2].tolist() == [3, 7] and (sc[:3, :2] == 1.0).all()
    assert all(q not in ids[r] for r, q in enumerate(query) if q > 0) and not np.isin(ids, [30, 31]).any()
    assert (ids[3:8] == 0).all() and np.isneginf(sc[3:8]).all() and (ids[8] == ids[9]).all()
    # k beyond the table: pads
    ids, sc = SR.similar_reference(torch.from_numpy(t), [3], 64, 'cos')
    assert (ids[0, :36] != 0).all() and (ids[0, 36:] == 0).all() and np.isneginf(sc[0, 36:]).all()      # 39 items - self - 2 dead


def test_floor_is_a_prefix_of_the_unfloored_list_and_ties_go_to_the_smaller_id():
    rng = np.random.default_rng(3)
    t = torch.from_numpy(SR.exact_cosine_table(rng, 500, 64))
    query = rng.integers(1, 500, size=20)
    full_i, full_s = SR.similar_reference(t, query, 499, 'cos')
    assert np.unique(full_s[full_i != 0]).size <= 33
    for r in range(20):                                                            # within equal scores the ids ascend
        n = int((full_i[r] != 0).sum())
        assert n == 498 and all(full_s[r, j] > full_s[r, j + 1] or full_i[r, j] < full_i[r, j + 1] for j in range(n - 1))
    for floor in (0.5, 0.25, 0.0, -0.0625):
        ids, sc = SR.similar_reference(t, query, 10, 'cos', min_sim=floor)
        for r in range(20):
            n = min(10, int((full_s[r] >= floor).sum()))
            assert ids[r, :n].tolist() == full_i[r, :n].tolist() and (ids[r, n:] == 0).all() and (sc[r, :n] >= floor).all()


def test_inverse_norms_of_the_restatement_and_the_stand_in():
    x = np.zeros((6, 64), np.float32)
    x[1, :4] = 1.0                                                                 # norm 2
    x[2, 0], x[3, 1], x[4, 2] = np.inf, np.nan, -np.inf
    x[5, :16] = 0.25                                                               # norm 1
    ref = SR.inv_norms_reference(torch.from_numpy(x))
    assert ref.dtype == np.float32 and ref.tolist() == [0.0, 0.5, 0.0, 0.0, 0.0, 1.0]
    out = torch.full((6,), 7.0)
    assert SR.sim_row_inv_norms(torch.from_numpy(x), out) is out and out.tolist() == ref.tolist()
    y = torch.from_numpy(np.random.default_rng(1).standard_normal((50, 128)).astype(np.float32))
    np.testing.assert_allclose(SR.inv_norms_reference(y), 1.0 / np.linalg.norm(y.numpy().astype(np.float64), axis=1), rtol=1e-7)


@pytest.mark.parametrize('K,E', [(10, 64), (100, 128), (256, 64), (32, 256), (10, 512)])
def test_random_cases_are_decided_by_the_restatement_alone(K, E):
    """The random cases of tests/test_similar_gpu.py from the restatement alone: 94 - 99 % of the positions are decided (the GPU test asks 90 %)."""
    rng = np.random.default_rng(K + E)
    t = torch.from_numpy(rng.standard_normal((14720, E)).astype(np.float32))
    query = rng.integers(1, 14720, size=64)
    _, rs = SR.similar_reference(t, query, K + 1, 'cos')
    share = float(SR.decided(rs, SR.cosine_bounds(t, query).max(1)).mean())
    print(f'K = {K}, E = {E}: {100 * share:.1f} % of the positions decided')
    assert 0.93 <= share <= 1.0


# ------------------------------------------------------------------ the flags
def test_both_parsers_take_the_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert (a.similar_out, a.similar_items, a.similar_metric, a.similar_min) == (None, None, 'cos', None)
        a = parse(['--mode', 'similar', '--topk', '20', '--similar_out', 'o.tsv', '--similar_items', 'q.txt', '--similar_metric', 'dot', '--similar_min', '0.95'])
        assert (a.mode, a.topk, a.similar_out, a.similar_items, a.similar_metric, a.similar_min) == ('similar', 20, 'o.tsv', 'q.txt', 'dot', 0.95)
        with pytest.raises(SystemExit):
            parse(['--similar_metric', 'l2'])
    with pytest.raises(SystemExit):
        parse_args(['--mode', 'neighbours'])


def test_flag_refusals():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    from adapter4rec_amd.data_utils.eval_flags import check_flags
    from adapter4rec_amd.parameters import parse_args
    for main in (run.main, run_adapter.main):
        for mode in ('train', 'test', 'recommend'):
            for flag in (['--similar_out', 'o.tsv'], ['--similar_items', 'q.txt'], ['--similar_metric', 'dot'], ['--similar_min', '0.9']):
                with pytest.raises(ValueError, match=f'{flag[0]} is honoured by --mode similar only, not by --mode {mode}'):
                    main(['--mode', mode] + flag)
        for flags, msg in ((['--candidate_lists', 'l.tsv'], '--candidate_lists'), (['--diversify', 'mmr'], '--diversify mmr'),
                           (['--eval_negatives', '100'], '--eval_negatives'), (['--similar_min', 'nan'], '--similar_min')):
            with pytest.raises(ValueError, match=msg):
                main(['--mode', 'similar'] + flags)
    with pytest.raises(ValueError, match='--similar_metric'):
        run.main(['--mode', 'load', '--similar_metric', 'dot'])
    for argv in (['--mode', 'similar'], ['--mode', 'similar', '--candidate_items', 'c.txt', '--similar_min=-inf', '--similar_metric', 'dot'],
                 ['--mode', 'train'], ['--mode', 'recommend', '--candidate_items', 'c.txt'], ['--mode', 'test', '--candidate_lists', 'l.tsv']):
        check_flags(parse_args(argv))                                              # what is honoured passes


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def _recording(item_emb, inv_norm, query, cand, min_sim, k, ids, scores):
    CALLS.append(dict(Q=int(query.numel()), cos=inv_norm is not None, cand=cand is not None, min_sim=min_sim, k=int(k), emb=item_emb))
    return SR.sim_topk_similar(item_emb, inv_norm, query, cand, min_sim, k, ids, scores)


def _refuse(*a, **k):
    raise AssertionError('a similar-item entry called under another mode')


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    norms = []

    def inv_norms(table, out=None):
        norms.append(table)
        return SR.sim_row_inv_norms(table, out)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', inv_norms, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_similar', _recording, raising=False)
    CALLS.clear()
    return norms


def _table(n=21, E=64, seed=5):
    t = torch.from_numpy(np.random.default_rng(seed).standard_normal((n, E)).astype(np.float32))
    t[6], t[13] = t[4] * 0.5, 0                                                    # a scaled twin of item 4 (cosine 1, another dot); a dead item
    return t


@pytest.mark.parametrize('metric', ('cos', 'dot'))
def test_similar_items_in_three_batches_against_the_restatement(simulated, monkeypatch, metric):
    from adapter4rec_amd.data_utils.metrics import similar_items
    emb = _table()
    N, k = emb.shape[0] - 1, 5
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '8')                                 # 20 queries: three batches
    ids, sc = similar_items(emb, k, metric=metric)
    assert [c['Q'] for c in CALLS] == [8, 8, 4] and all(c['cos'] == (metric == 'cos') and not c['cand'] and c['min_sim'] is None for c in CALLS)
    assert len(simulated) == (metric == 'cos')                                     # the inverse norms: once per call, not per batch
    assert ids.dtype == torch.long and sc.dtype == torch.float32 and tuple(ids.shape) == (N, k) == tuple(sc.shape)
    ri, rs = SR.similar_reference(emb, np.arange(1, N + 1), k, metric)
    np.testing.assert_array_equal(ids.numpy(), ri)
    np.testing.assert_allclose(sc.numpy(), rs, rtol=0, atol=1e-5)
    if metric == 'cos':
        assert ids[3, 0] == 6 and ids[5, 0] == 4 and (ids[12] == 0).all() and torch.isneginf(sc[12]).all() and not (ids == 13).any()
    # a query list: its order, repeats, ids that are no item; candidates; the floor
    CALLS.clear()
    cand = np.random.default_rng(6).random(N + 1) < 0.5
    query = torch.tensor([9, 2, 2, 0, N + 1, 17, -3, 4])
    ids, sc = similar_items(emb, k, item_ids=query, candidates=cand, metric=metric, min_sim=0.05)
    assert [c['Q'] for c in CALLS] == [8] and CALLS[0]['cand'] and CALLS[0]['min_sim'] == 0.05 and CALLS[0]['k'] == k
    ri, rs = SR.similar_reference(emb, query, k, metric, cand=cand, min_sim=0.05)
    np.testing.assert_array_equal(ids.numpy(), ri)
    assert cand[ids[ids != 0].numpy()].all() and (ids[[3, 4, 6]] == 0).all() and torch.equal(ids[1], ids[2])
    assert tuple(similar_items(emb, k, item_ids=[], metric=metric)[0].shape) == (0, k)
    for kw, msg in ((dict(metric='l2'), 'metric'), (dict(min_sim=float('nan')), 'min_sim'), (dict(candidates=np.zeros(N + 1, bool)), 'no candidate'),
                    (dict(candidates=np.ones(N, bool)), 'one entry per table row')):
        with pytest.raises(ValueError, match=msg):
            similar_items(emb, k, **kw)


def test_write_similar_items_file_and_log(simulated, monkeypatch, tmp_path):
    from adapter4rec_amd.data_utils.metrics import read_similar_items, write_similar_items
    emb = _table()
    N, k = emb.shape[0] - 1, 4
    names = [None] + [f'I{i:02d}' for i in range(1, N + 1)]
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '8')
    path, log = str(tmp_path / 'all.tsv'), _Log()
    assert write_similar_items(emb, k, 16, names, path, Log_file=log) == path       # every item, sharded at batch size 16: the sampler pads the tail
    ri, rs = SR.similar_reference(emb, np.arange(1, N + 1), k, 'cos')
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    assert [r[0] for r in rows] == [names[i] for i in range(1, N + 1) if i != 13]    # query order; the dead item has no neighbour: no line
    for r in rows:
        i = names.index(r[0])
        assert r[1].split(' ') == [names[j] for j in ri[i - 1]] and len(r) == 3
        got = np.array([np.float32(x) for x in r[2].split(' ')])
        np.testing.assert_allclose(got, rs[i - 1], rtol=0, atol=1e-5)
        assert all('%.9g' % float(x) == s for x, s in zip(got, r[2].split(' ')))
    best = np.mean([rs[i - 1, 0] for i in range(1, N + 1) if i != 13])
    assert len(log.lines) == 1
    m = re.fullmatch(r'similar   top-4 lists of 20 items, 19 with a neighbour, mean best score (\d\.\d{5}) -> (.*)', log.lines[0])
    assert m and m.group(2) == path and abs(float(m.group(1)) - best) < 2e-5
    # --similar_items: file order, blanks and repeats ignored, unknown names raise
    qfile = tmp_path / 'q.txt'
    qfile.write_text('I09\n\nI02\nI09\n  I13  \nI20\n')
    query = read_similar_items(str(qfile), names)
    assert query.tolist() == [9, 2, 13, 20]
    path2 = str(tmp_path / 'some.tsv')
    write_similar_items(emb, k, 16, names, path2, item_ids=query, metric='dot', min_sim=1.0, Log_file=log)
    rows = [l.rstrip('\n').split('\t') for l in open(path2)]
    ri, rs = SR.similar_reference(emb, query, k, 'dot', min_sim=1.0)
    keep = [r for r in range(4) if ri[r, 0] != 0]
    assert [r[0] for r in rows] == [names[int(query[r])] for r in keep] and 0 < len(keep)
    for row, r in zip(rows, keep):
        assert row[1].split(' ') == [names[j] for j in ri[r] if j != 0] and len(row[2].split(' ')) == int((ri[r] != 0).sum())
    assert log.lines[1].startswith(f'similar   top-4 lists of 4 items, {len(keep)} with a neighbour')
    qfile.write_text('I09\nnope\nI02\nnada\n')
    with pytest.raises(ValueError, match='2 name.s. that are no item of this dataset: nope, nada'):
        read_similar_items(str(qfile), names)
    qfile.write_text('\n\n')
    with pytest.raises(ValueError, match='no item name'):
        read_similar_items(str(qfile), names)


def test_other_modes_never_call_the_new_entries(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users, sim_topk_items_cand
    from topk_ref import sim_topk_items
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend, write_recommendations
    monkeypatch.setattr(sim_lib, 'topk_similar', _refuse)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', _refuse)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand, raising=False)
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(12)
    seqs = {u: eval_seq[u][:-1] for u in eval_seq}
    recommend(model, seqs, emb, 5, args)
    recommend(model, seqs, emb, 5, args, candidates=np.ones(item_num + 1, bool))
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    write_recommendations(model, eval_seq, hist, emb, 5, 16, args, [f'U{u}' for u in seqs], names, str(tmp_path / 'r.tsv'), Log_file=_Log())
    eval_model(model, hist, eval_seq, emb, 16, args, item_num, logging.getLogger('t'), 'test', 0)
    from adapter4rec_amd.data_utils.metrics import similar_items
    with pytest.raises(AssertionError, match='similar-item entry called'):
        similar_items(emb, 5)


# ------------------------------------------------------------------ the entry points
def _check_file(path, emb, item_names, query, k, metric, cand=None, floor=None):
    """every line of a --mode similar file against the stand-in's own lists on the table the run computed"""
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(torch.int32)
    ids = torch.zeros(q.numel(), k, dtype=torch.int32)
    sc = torch.zeros(q.numel(), k)
    inv = SR.sim_row_inv_norms(emb) if metric == 'cos' else None
    SR.sim_topk_similar(emb, inv, q, None if cand is None else torch.from_numpy(cand.astype(np.uint8)), floor, k, ids, sc)
    ids, sc = ids.numpy(), sc.numpy()
    want = []
    for r in range(q.numel()):
        keep = ids[r] != 0
        if keep.any():
            want.append([item_names[int(q[r])], ' '.join(item_names[int(i)] for i in ids[r][keep]), ' '.join('%.9g' % float(s) for s in sc[r][keep])])
    got = [l.rstrip('\n').split('\t') for l in open(path)]
    assert got == want and len(got) > 0
    return got


def test_text_runner_mode_similar(tmp_path, monkeypatch):
    """train one epoch through run.py and recommend from its checkpoint with the new entries refusing every call; then --mode similar from the same
    checkpoint: every item by cosine to the default path, then a query file within a candidate file by dot product with a floor"""
    import test_text_run as TR
    import test_topk_cpu as TC
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    TC._simulated(monkeypatch)
    monkeypatch.setattr(sim_lib, 'topk_similar', _refuse, raising=False)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', _refuse, raising=False)
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'sim']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    TR._run(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '3'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    kept = []

    def keeping(item_emb, inv_norm, query, cand, min_sim, k, ids, scores):
        kept.append(item_emb.clone())
        return SR.sim_topk_similar(item_emb, inv_norm, query, cand, min_sim, k, ids, scores)
    monkeypatch.setattr(sim_lib, 'topk_similar', keeping)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', SR.sim_row_inv_norms)
    import adapter4rec_amd.data_utils.metrics as M
    monkeypatch.setattr(M, '_recommend', lambda *a, **k: pytest.fail('--mode similar touched the users'))
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    from adapter4rec_amd import run
    orig_setup = run.setuplogger

    def setup(*a, **kw):                                                          # (TR._run drops the loggers' handlers after every run)
        out = orig_setup(*a, **kw)
        logging.getLogger('Log_file').addHandler(Keep())
        return out
    monkeypatch.setattr(run, 'setuplogger', setup)
    rec = dict(loss=[], batch=[], eval=[])
    TR._run(common + ['--mode', 'similar', '--load_ckpt_name', 'epoch-1.pt', '--topk', '4'], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == []                                # no training step, no evaluation
    out = os.path.join(os.path.dirname(ck[0]), 'similar_epoch-1.pt.tsv')
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    _, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    N = len(item_names) - 1
    emb = kept[0]
    assert tuple(emb.shape) == (N + 1, 64)
    rows = _check_file(out, emb, item_names, np.arange(1, N + 1), 4, 'cos')
    assert [r[0] for r in rows] == item_names[1:] and all(len(r[1].split(' ')) == 4 for r in rows)
    line = [l for l in seen if l.startswith('similar   ')]
    assert len(line) == 1 and line[0].startswith(f'similar   top-4 lists of {N} items, {N} with a neighbour, mean best score ') and line[0].endswith('/similar_epoch-1.pt.tsv')
    # a query file, a candidate file, the dot metric, a floor, another path
    q_names, c_names = [item_names[i] for i in (7, 3, 7, 11)], [item_names[i] for i in range(1, N + 1) if i % 3]
    open(os.path.join(root, 'q.txt'), 'w').write('\n'.join(q_names) + '\n')
    open(os.path.join(root, 'c.txt'), 'w').write('\n'.join(c_names) + '\n')
    cand = np.zeros(N + 1, bool)
    cand[[i for i in range(1, N + 1) if i % 3]] = True
    dots = (emb @ emb.t()).numpy()
    floor = float(np.median(dots[7, 1:]))
    out2 = os.path.join(root, 'some.tsv')
    TR._run(common + ['--mode', 'similar', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--similar_out', out2, '--similar_items', os.path.join(root, 'q.txt'),
                      '--candidate_items', os.path.join(root, 'c.txt'), '--similar_metric', 'dot', '--similar_min', repr(floor)], monkeypatch, rec)
    rows = _check_file(out2, emb, item_names, [7, 3, 11], 5, 'dot', cand, floor)
    assert all(set(r[1].split(' ')) <= set(c_names) for r in rows) and all(float(s) >= np.float32(floor) for r in rows for s in r[2].split(' '))
    assert any(l.startswith(f'similar items: 3 of {N} from ') for l in seen) and any(l.startswith(f'candidate items: {len(c_names)} of {N} from ') for l in seen)
    assert torch.equal(kept[-1], emb)                                              # the same table from the same checkpoint


def test_cv_id_runner_mode_similar(tmp_path, monkeypatch):
    """the image entry point with --item_tower id: train one epoch with the new entries refusing every call, then --mode similar from its checkpoint:
    the neighbours of the ID table's rows"""
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    from topk_ref import sim_topk_items
    from adapter4rec_amd.cv.data_utils import read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    for n in ('id_index', 'id_grad_sum', 'id_index_ws_ints'):
        if hasattr(IC, n):
            monkeypatch.setattr(sim_lib, n, getattr(IC, n), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_similar', _refuse, raising=False)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', _refuse, raising=False)
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    monkeypatch.setattr(sim_lib, 'topk_similar', SR.sim_topk_similar)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', SR.sim_row_inv_norms)
    out = os.path.join(root, 'sim.tsv')
    CR._run_cv(common + ['--mode', 'similar', '--load_ckpt_name', 'epoch-1.pt', '--topk', '6', '--similar_out', out, '--similar_min', '0.0'], monkeypatch,
               dict(loss=[], batch=[], eval=[]))
    keys, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    _, item_names = read_behavior_names(os.path.join(data, 'toy', 'users_log.tsv'), name2id, 20, 5)
    N = len(item_names) - 1
    emb = torch.load(ck[0], map_location='cpu', weights_only=False)['model_state_dict']['id_embedding.weight'].float()
    assert emb.shape[0] == N + 1
    rows = _check_file(out, emb, item_names, np.arange(1, N + 1), 6, 'cos', floor=0.0)
    ri, rs = SR.similar_reference(emb, np.arange(1, N + 1), 6, 'cos', min_sim=0.0)       # and the fp64 restatement where it is decided
    sure = SR.decided(SR.similar_reference(emb, np.arange(1, N + 1), 7, 'cos')[1], SR.cosine_bounds(emb, np.arange(1, N + 1)).max(1))
    by_name = {r[0]: r[1].split(' ') for r in rows}
    checked = 0
    for i in range(1, N + 1):
        got = by_name.get(item_names[i], [])
        for j in range(min(len(got), int((ri[i - 1] != 0).sum()))):
            if sure[i - 1, :j + 1].all() and rs[i - 1, j] > 1e-6:
                assert got[j] == item_names[int(ri[i - 1, j])], (i, j)
                checked += 1
    assert checked > N
