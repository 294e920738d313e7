"""CPU side of the diversified re-ranking (include/a4r_diversify.h: a4r_mmr_rerank): the C boundary of the export (header, the binding's table in
adapter4rec_amd/_lib_diversify.py, the built library, refusals in front of the first HIP call), the properties of the rule on its restatement
(tests/mmr_ref.py), the flags in both parsers and their refusals, and recommend / write_recommendations / the text runner on the stand-in library
against the restatement."""
import ctypes
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import lists_ref as LR
import mmr_ref as MR
import sim_lib
from topk_ref import sim_topk_items

NAMES = ['a4r_mmr_rerank']
HEADER = ('include', 'a4r_diversify.h')


# ------------------------------------------------------------------ the C boundary, held as tests/test_eval_negatives_cpu.py holds its header
def mmr_prototypes():
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
    protos = mmr_prototypes()
    table = L.DIVERSIFY_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    assert not set(table) & (set(L.SIGNATURES) | set(L.SCORE_CE_BF16_SIGNATURES) | set(L.CANDIDATES_SIGNATURES) | set(L.USER_LISTS_SIGNATURES)
                             | set(L.EVAL_NEGATIVES_SIGNATURES))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert table['a4r_mmr_rerank'] == (_I, (_P,) * 7 + (_F,) + (_I,) * 5)
    txt = ABI.header(HEADER)
    assert dict(re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt)) == {'A4R_MMR_MAX_POOL': '256'}
    assert L.MMR_MAX_POOL == MR.MAX_POOL == L.TOPK_MAX_K == 256 and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    assert 'smaller pool position' in raw and 'never dereferenced' in raw        # the tie rule and the validity rule are written down
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert a4r_h.count('#include "a4r_diversify.h"') == 1
    assert a4r_h.index('#include "a4r_user_lists.h"') < a4r_h.index('#include "a4r_diversify.h"')
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_mmr_rerank(*([None] * 7), 'half', 1, 2, 64, 1, 1)
    mk = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'Makefile')).read()
    assert 'a4r_mmr.hip' in mk and mk.count('../../include/a4r_diversify.h') == 3  # the source, and the header in the three dependency lists


def test_wrapper_is_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_diversify as B
    assert L.mmr_rerank is B.mmr_rerank and L.DIVERSIFY_SIGNATURES is B.DIVERSIFY_SIGNATURES and L.MMR_MAX_POOL == B.MMR_MAX_POOL


def test_export_refuses_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (nothing is enqueued, no GPU is needed): each pointer in turn NULL -- all but the stream and ild,
    whose NULL means "not wanted" and is therefore only probed beside another bad argument -- then U < 1, N1 < 2, E not served, P outside
    1 .. 256, K outside 1 .. P, lambda outside [0, 1] or NaN, and item_emb off a 16-byte boundary."""
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    f = lib.a4r_mmr_rerank
    f.restype, f.argtypes = L.DIVERSIFY_SIGNATURES['a4r_mmr_rerank']
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    # (stream, item_emb, pool_ids, pool_scores, ids, scores, ild, lambda, U, N1, E, P, K)
    good = [None, p, p, p, p, p, p, 0.5, 4, 100, 64, 20, 10]
    probed = 0
    for i in (1, 2, 3, 4, 5):
        for ild in (p, None):
            a = list(good)
            a[i], a[6] = None, ild
            assert f(*a) == -1, i
        probed += 1
    bad = [(8, 0), (8, -1), (9, 1), (9, 0), (9, -5), (10, 0), (10, 32), (10, 96), (10, 1024), (10, -64), (11, 0), (11, -1), (11, 257), (12, 0),
           (12, -1), (12, 21), (12, 257), (7, -0.001), (7, 1.001), (7, float('nan')), (7, float('inf')), (7, -float('inf'))]
    for i, v in bad:
        for ild in (p, None):
            a = list(good)
            a[i], a[6] = v, ild
            assert f(*a) == -1, (i, v)
        probed += 1
    for off in (4, 8, 12):
        a = list(good)
        a[1] = p + off
        assert f(*a) == -1, off
    assert f(*([None] * 7), 0.0, 0, 0, 0, 0, 0) == -1
    assert probed == 5 + len(bad)


def test_wrapper_refuses_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, U, E, P, k = 9, 4, 64, 6, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(item_emb=torch.zeros(N1, E), pool_ids=i32(U, P), pool_scores=torch.zeros(U, P), lam=0.5, k=k, ids=i32(U, k), scores=torch.zeros(U, k),
                ild=torch.zeros(U))
    call = lambda **kw: L.mmr_rerank(**dict(good, **kw))
    wide = torch.zeros(N1, 2 * E)[:, :E]
    off = torch.zeros(N1 * E + 1)[1:].view(N1, E)
    assert off.data_ptr() % 16 == 4 and not wide.is_contiguous()
    for kw, msg in [(dict(item_emb=torch.zeros(N1, E, dtype=torch.float64)), 'item_emb'), (dict(item_emb=wide), 'item_emb'), (dict(item_emb=off), 'aligned'),
                    (dict(item_emb=torch.zeros(N1, 96)), 'E = 96'), (dict(item_emb=torch.zeros(1, E)), 'N1 = 1'), (dict(item_emb=torch.zeros(N1 * E)), 'expected'),
                    (dict(pool_ids=i32(U, P).long()), 'pool_ids'), (dict(pool_ids=i32(U, P + 1)), 'expected'), (dict(pool_ids=i32(U * P)), 'expected'),
                    (dict(pool_scores=torch.zeros(U, P, dtype=torch.float64)), 'pool_scores'), (dict(pool_ids=i32(U, 2 * P)[:, :P]), 'pool_ids'),
                    (dict(pool_ids=i32(U, 257), pool_scores=torch.zeros(U, 257)), 'P = 257'), (dict(pool_ids=i32(0, P), pool_scores=torch.zeros(0, P)), 'U = 0'),
                    (dict(k=0), 'k = 0'), (dict(k=P + 1), 'k = 7'), (dict(lam=-0.1), 'lambda'), (dict(lam=1.5), 'lambda'), (dict(lam=float('nan')), 'lambda'),
                    (dict(ids=i32(U, k + 1)), 'ids and scores'), (dict(ids=i32(U, k).long()), 'ids'), (dict(scores=torch.zeros(U + 1, k)), 'ids and scores'),
                    (dict(scores=torch.zeros(U, k, dtype=torch.float64)), 'scores'), (dict(ild=torch.zeros(U + 1)), 'ild'), (dict(ild=torch.zeros(U, 1)), 'ild'),
                    (dict(ild=torch.zeros(U, dtype=torch.float64)), 'ild')]:
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(RuntimeError, match='device tensors'):
        monkeypatch.undo()
        L.mmr_rerank(**good)                                                       # host tensors never reach a kernel


# ------------------------------------------------------------------ the rule itself, on the restatement
def test_lambda_one_gives_the_valid_prefix():
    t = MR.exact_table(300, 64)
    pid, ps = MR.exact_pool(3, 100, 300, 1)
    order = np.argsort(-np.where(np.isfinite(ps), ps, -np.inf), axis=1, kind='stable')         # a pool as top-K leaves it: sorted, pads last
    pid, ps = np.take_along_axis(pid, order, 1), np.take_along_axis(ps, order, 1)
    for k in (1, 10, 100):
        ids, sc, ild, _, _ = MR.mmr_reference(t, pid, ps, 1.0, k)
        for u in range(3):
            ok = np.flatnonzero((pid[u] >= 1) & (pid[u] < 300) & np.isfinite(ps[u]))[:k]
            assert ids[u, :ok.size].tolist() == pid[u, ok].tolist() and sc[u, :ok.size].tolist() == ps[u, ok].tolist()
            assert (ids[u, ok.size:] == 0).all() and np.isneginf(sc[u, ok.size:]).all()
    # an unsorted pool under lambda = 1: by score, ties by position
    ids, sc, *_ = MR.mmr_reference(t, [[11, 12, 13, 14]], [[1.0, 5.0, 5.0, 2.0]], 1.0, 4)
    assert ids.tolist() == [[12, 13, 14, 11]] and sc.tolist() == [[5.0, 5.0, 2.0, 1.0]]


def test_each_round_maximises_v_by_brute_force():
    """every pick, recomputed from the definition over all valid unselected entries with the similarities formed pair by pair"""
    rng = np.random.default_rng(3)
    N1, E, P, K = 50, 64, 24, 12
    emb = rng.standard_normal((N1, E))
    emb[9] = 0
    for lam in (0.0, 0.3, 0.7, 1.0):
        pid = rng.integers(-2, N1 + 3, size=P)
        ps = rng.uniform(-3, 3, size=P)
        ps[5], ps[6] = np.nan, np.inf
        ids, sc, ild, margins, picks = MR.mmr_user(emb, pid, ps, lam, K)
        valid = [j for j in range(P) if 1 <= pid[j] < N1 and math.isfinite(ps[j])]
        assert 2 <= len(valid) < P and set(picks) <= set(valid) and len(set(picks)) == len(picks) == min(K, len(valid))
        lo, hi = min(ps[j] for j in valid), max(ps[j] for j in valid)

        def cos(i, j):
            a, b = emb[pid[i]], emb[pid[j]]
            na, nb = math.sqrt(float(a @ a)), math.sqrt(float(b @ b))
            return float(a @ b) / (na * nb) if na > 0 and nb > 0 else 0.0
        for t, b in enumerate(picks):
            v = {j: lam * (ps[j] - lo) / (hi - lo) - (1 - lam) * max([cos(i, j) for i in picks[:t]], default=0.0) for j in valid if j not in picks[:t]}
            best = max(v.values())
            assert v[b] >= best - 1e-12 and min(j for j in v if v[j] >= best - 1e-12) == b, (lam, t)
            others = sorted(v.values())[:-1]
            assert (abs(margins[t] - (v[b] - others[-1])) < 1e-12) if others else np.isinf(margins[t])
            assert ids[t] == pid[b] and sc[t] == ps[b]
        pairs = [(i, j) for n, i in enumerate(picks) for j in picks[:n]]
        assert abs(ild - sum(1 - cos(i, j) for i, j in pairs) / len(pairs)) < 1e-12


def test_ties_duplicates_zero_norm_and_range_zero():
    t = MR.exact_table(300, 64).astype(np.float64)
    a, b = MR.TWINS
    z = MR.ZERO_ROW
    other = 20
    c_ab = float(t[a] @ t[other]) / (math.sqrt(float(t[a] @ t[a])) * math.sqrt(float(t[other] @ t[other])))
    assert (t[a] == t[b]).all() and not t[z].any() and abs(c_ab) < 1
    # the near-duplicate case: the twin of pick 1 has the second-best score and is not pick 2 at lambda = 0.5; at lambda = 1 it is
    pool, sc = [a, b, other, z], [8.0, 7.0, 4.0, 0.0]
    ids, s, ild, _, picks = MR.mmr_user(t, pool, sc, 0.5, 4)
    assert ids[0] == a and ids[1] != b and sorted(ids.tolist()) == sorted(pool) and s.tolist() == [sc[j] for j in picks]
    assert MR.mmr_user(t, pool, sc, 1.0, 4)[0].tolist() == pool
    # a zero-norm row has cosine 0 to everything: after pick 1 it loses nothing, so at lambda = 0 it beats every row with a positive cosine
    ids0 = MR.mmr_user(t, [a, b, z], [3.0, 2.0, 1.0], 0.0, 3)[0]
    assert ids0.tolist() == [a, z, b]                                             # round 0: all v = 0, the smallest position; then z (0) over b (-1)
    # a repeated id is two entries with cosine 1, and both can be returned
    ids, s, ild, *_ = MR.mmr_user(t, [a, a], [2.0, 1.0], 0.5, 2)
    assert ids.tolist() == [a, a] and s.tolist() == [2.0, 1.0] and abs(ild) < 1e-15
    # ties go to the smaller pool position: equal scores, equal rows
    assert MR.mmr_user(t, [b, a, b], [1.0, 1.0, 1.0], 0.5, 3)[4] == [0, 1, 2]
    # range 0: r = 1 for every valid entry, whatever the score; one valid entry likewise
    ids, s, *_ = MR.mmr_user(t, [other, 0, a, 999], [5.0, -np.inf, 5.0, 5.0], 0.25, 4)
    assert ids.tolist() == [other, a, 0, 0] and s[:2].tolist() == [5.0, 5.0] and np.isneginf(s[2:]).all()
    v_first = 0.25 * 1.0
    assert MR.mmr_user(t, [other, a], [5.0, 5.0], 0.25, 2)[3][0] == 0.0 and v_first == 0.25          # both r = 1: an exact tie in round 0
    # nothing valid: pads only, ild 0
    ids, s, ild, margins, picks = MR.mmr_user(t, [0, -1, 300, a], [1.0, 1.0, 1.0, np.nan], 0.5, 3)
    assert ids.tolist() == [0, 0, 0] and np.isneginf(s).all() and ild == 0.0 and picks == [] and np.isinf(margins).all()
    # fewer than two picks: ild 0
    assert MR.mmr_user(t, [a, 0], [1.0, -np.inf], 0.5, 2)[2] == 0.0


@pytest.mark.parametrize('E', (64, 512))
def test_random_case_is_decided_by_the_margin_rule(E):
    """The random case of tests/test_mmr_gpu.py, from the restatement alone: at most 10 % of the users have a round whose margin is below tau."""
    emb, pid, ps = MR.gaussian_case(E)
    _, _, _, margin, _ = MR.mmr_reference(emb, pid, ps, 0.7, 10)
    share = float((margin <= MR.tau(E)).mean())
    print(f'E = {E}: tau = {MR.tau(E):.3g}, {100 * share:.1f} % of 64 users under it, smallest margin {margin.min():.3g}')
    assert share <= 0.10


# ------------------------------------------------------------------ the flags
def test_both_parsers_take_the_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert (a.diversify, a.mmr_lambda, a.mmr_pool) == ('none', 0.7, 100)
        a = parse(['--mode', 'recommend', '--diversify', 'mmr', '--mmr_lambda', '0.4', '--mmr_pool', '50'])
        assert (a.diversify, a.mmr_lambda, a.mmr_pool) == ('mmr', 0.4, 50)
        with pytest.raises(SystemExit):
            parse(['--diversify', 'dpp'])


def test_flag_refusals():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    from adapter4rec_amd.data_utils.eval_flags import check_diversify_flag
    from adapter4rec_amd.data_utils.metrics import Diversify
    from adapter4rec_amd.parameters import parse_args
    for main in (run.main, run_adapter.main):
        for mode in ('train', 'test'):
            with pytest.raises(ValueError, match='--diversify mmr is honoured by --mode recommend only'):
                main(['--mode', mode, '--diversify', 'mmr'])
        for lam in ('-0.1', '1.5', 'nan'):
            with pytest.raises(ValueError, match='--mmr_lambda'):
                main(['--mode', 'recommend', '--diversify', 'mmr', '--mmr_lambda', lam])
        for pool, topk in (('9', '10'), ('257', '10'), ('0', '10'), ('100', '101')):
            with pytest.raises(ValueError, match='--mmr_pool'):
                main(['--mode', 'recommend', '--diversify', 'mmr', '--mmr_pool', pool, '--topk', topk])
    with pytest.raises(ValueError, match='--diversify'):
        run.main(['--mode', 'load', '--diversify', 'mmr'])
    check_diversify_flag(parse_args(['--mode', 'train', '--mmr_lambda', '7', '--mmr_pool', '1']))          # without --diversify mmr nothing is looked at
    for topk, pool in ((10, 10), (10, 256), (256, 256)):
        check_diversify_flag(parse_args(['--mode', 'recommend', '--diversify', 'mmr', '--topk', str(topk), '--mmr_pool', str(pool), '--mmr_lambda', '1']))
    for lam, pool in ((-0.1, 10), (float('nan'), 10), (0.5, 0), (0.5, 257)):
        with pytest.raises(ValueError, match='diversify'):
            Diversify(lam, pool)
    assert (Diversify().lam, Diversify().pool) == (0.7, 100)


# ------------------------------------------------------------------ the Python API on simulated kernels
POOLS = []


def _recording(fn, ids_at, scores_at):
    def wrapped(*a):
        out = fn(*a)
        POOLS.append((a[ids_at].clone(), a[scores_at].clone()))
        return out
    return wrapped


def _refuse(*a, **k):
    raise AssertionError('mmr_rerank called without diversify / a top-K entry of another mode called')


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
    from test_candidates_cpu import sim_topk_items_cand
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'topk_items', _recording(sim_topk_items, 5, 6), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', _recording(sim_topk_items_cand, 6, 7), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_lists', _recording(LR.sim_topk_lists, 8, 9), raising=False)
    monkeypatch.setattr(sim_lib, 'mmr_rerank', MR.sim_mmr_rerank, raising=False)
    POOLS.clear()


def _with_twins(emb, item_num):
    """the fixture's table with near-duplicates in it: every odd item a copy of the even item before it (scaled: another score, cosine 1)"""
    emb = emb.clone()
    for i in range(2, item_num, 2):
        emb[i + 1] = emb[i] * 0.97
    return emb


@pytest.mark.parametrize('mode', ('full', 'candidates', 'candidate_lists'))
def test_recommend_diversified_against_the_restatement(simulated, monkeypatch, mode, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(21)
    emb = _with_twins(emb, item_num)
    U, k, pool, lam = len(eval_seq), 5, 16, 0.5
    rng = np.random.default_rng(31)
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    kw = {}
    if mode == 'candidates':
        mask = rng.random(item_num + 1) < 0.7
        mask[1:4] = True
        kw = dict(candidates=mask)
    elif mode == 'candidate_lists':
        kw = dict(candidate_lists={u: [int(x) for x in rng.integers(-1, item_num + 3, size=int(rng.integers(0, 41)))] for u in range(U) if u % 4 != 1})
    used = dict(full='topk_items', candidates='topk_items_cand', candidate_lists='topk_lists')[mode]
    for name in ('topk_items', 'topk_items_cand', 'topk_lists'):
        if name != used:
            monkeypatch.setattr(sim_lib, name, _refuse, raising=False)
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '8')                                 # three batches
    spec = Diversify(lam, pool)
    ids, sc = recommend(model, seqs, emb, k, args, diversify=spec, **kw)
    assert len(POOLS) == 3 and all(p[0].shape[1] == pool for p in POOLS)          # the mode's entry ran with k = pool
    pool_i, pool_s = torch.cat([p[0] for p in POOLS]).numpy(), torch.cat([p[1] for p in POOLS]).numpy()
    ri, rs, rild, _, _ = MR.mmr_reference(emb.numpy(), pool_i, pool_s, lam, k)
    assert ids.dtype == torch.long and tuple(ids.shape) == (U, k) == tuple(sc.shape)
    np.testing.assert_array_equal(ids.numpy(), ri)
    np.testing.assert_array_equal(sc.numpy(), rs.astype(np.float32))
    plain_i = MR.mmr_reference(emb.numpy(), pool_i, pool_s, 1.0, k)[0]
    np.testing.assert_array_equal(plain_i, pool_i[:, :k])
    assert (ri != plain_i).any()                                                   # the re-ranking changes lists here
    POOLS.clear()
    p_ids, p_sc = recommend(model, seqs, emb, k, args, **kw)                      # without diversify: the plain list, the entry run with k
    assert all(p[0].shape[1] == k for p in POOLS)
    np.testing.assert_array_equal(p_ids.numpy(), plain_i)
    with pytest.raises(ValueError, match='k = 17 outside 1 .. pool = 16'):
        recommend(model, seqs, emb, 17, args, diversify=spec, **kw)
    # the file and the log line
    user_names = [f'U{u}' for u in range(U)]
    item_names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    path = str(tmp_path / 'rec.tsv')
    log = _Log()
    POOLS.clear()
    assert write_recommendations(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, diversify=spec, Log_file=log, **kw) == path
    pool_i, pool_s = torch.cat([p[0] for p in POOLS]).numpy()[:U], torch.cat([p[1] for p in POOLS]).numpy()[:U]     # (the sampler pads its last batch)
    ri, rs, d_mmr, _, _ = MR.mmr_reference(emb.numpy(), pool_i, pool_s, lam, k)
    d_plain = MR.mmr_reference(emb.numpy(), pool_i, pool_s, 1.0, k)[2]
    rows = {r[0]: r for r in (l.rstrip('\n').split('\t') for l in open(path))}
    listed = [u for u in range(U) if mode != 'candidate_lists' or u in kw['candidate_lists']]
    assert sorted(rows) == sorted(f'U{u}' for u in listed)
    for u in listed:
        keep = ri[u] != 0
        assert rows[f'U{u}'][1] == ' '.join(f'N{i}' for i in ri[u][keep])
        assert rows[f'U{u}'][2] == ' '.join('%.9g' % float(np.float32(s)) for s in rs[u][keep])
    two = (ri != 0).sum(1) >= 2
    line = [l for l in log.lines if l.startswith('recommend_ild')]
    assert len(line) == 1 and line[0].endswith(f'{int(two.sum())} of {U} users') and f'top-{k} ' in line[0] and 'mmr(lambda 0.5, pool 16)' in line[0]
    got = [float(x) for x in re.findall(r' (\d\.\d{5})', line[0])]
    np.testing.assert_allclose(got, [d_plain[two].mean(), d_mmr[two].mean()], atol=2e-5)
    assert got[1] > got[0]                                                         # the re-ranked lists are the more diverse
    if mode == 'candidate_lists':
        assert int(two.sum()) < U
    log2 = _Log()
    write_recommendations(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, Log_file=log2, **kw)
    assert not log2.lines                                                          # no flag: no line


def test_without_the_flag_mmr_rerank_is_never_called(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(12)
    seqs = {u: eval_seq[u][:-1] for u in eval_seq}
    monkeypatch.setattr(sim_lib, 'mmr_rerank', _refuse)
    a = recommend(model, seqs, emb, 5, args)
    b = recommend(model, seqs, emb, 5, args, diversify=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    recommend(model, seqs, emb, 5, args, candidates=np.ones(item_num + 1, bool))
    recommend(model, seqs, emb, 5, args, candidate_lists={u: [1, 2, 3] for u in seqs})
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    write_recommendations(model, eval_seq, hist, emb, 5, 16, args, [f'U{u}' for u in seqs], names, str(tmp_path / 'r.tsv'), Log_file=_Log())
    with pytest.raises(AssertionError, match='mmr_rerank called'):
        recommend(model, seqs, emb, 5, args, diversify=Diversify(0.5, 8))
    # lambda = 1 through the real path is the plain list
    monkeypatch.setattr(sim_lib, 'mmr_rerank', MR.sim_mmr_rerank)
    c = recommend(model, seqs, emb, 5, args, diversify=Diversify(1.0, 8))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ------------------------------------------------------------------ the text entry point
def test_text_runner_recommend_diversified(tmp_path, monkeypatch):
    """train one epoch through run.py, then --mode recommend with and without --diversify mmr from its checkpoint: the diversified file is the
    restatement's re-ranking of the pool the plain run with --topk = the pool size writes, and the ILD line is logged."""
    import logging
    import test_text_run as TR
    import test_topk_cpu as TC
    TC._simulated(monkeypatch)
    monkeypatch.setattr(sim_lib, 'mmr_rerank', MR.sim_mmr_rerank, raising=False)
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'mmr']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    assert len(glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))) == 1
    pool, k, lam = 12, 4, 0.0            # (the toy tower's item vectors are all but collinear after one epoch: only a pure-diversity run reorders them)
    plain, div = os.path.join(root, 'pool.tsv'), os.path.join(root, 'div.tsv')
    rec = ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt']
    kept = {}
    real = sim_lib.mmr_rerank

    def keeping(item_emb, pool_ids, pool_scores, lam_, k_, ids, scores, ild=None):
        kept.setdefault('emb', item_emb.clone())
        kept.setdefault('calls', []).append((float(lam_), int(k_), ild is not None))
        return real(item_emb, pool_ids, pool_scores, lam_, k_, ids, scores, ild)
    monkeypatch.setattr(sim_lib, 'mmr_rerank', keeping)
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    handler = Keep()
    from adapter4rec_amd import run
    orig_setup = run.setuplogger

    def setup(*a, **kw):                                                          # (TR._run drops the loggers' handlers after every run)
        out = orig_setup(*a, **kw)
        logging.getLogger('Log_file').addHandler(handler)
        return out
    monkeypatch.setattr(run, 'setuplogger', setup)
    TR._run(common + rec + ['--recommend_out', plain, '--topk', str(pool)], monkeypatch, dict(loss=[], batch=[], eval=[]))
    assert 'calls' not in kept and not any(l.startswith('recommend_ild') for l in seen)          # no flag: no call, no line
    TR._run(common + rec + ['--recommend_out', div, '--topk', str(k), '--diversify', 'mmr', '--mmr_lambda', str(lam), '--mmr_pool', str(pool)],
            monkeypatch, dict(loss=[], batch=[], eval=[]))
    assert kept['calls'] and set(kept['calls']) == {(1.0, k, True), (lam, k, True)} and len(kept['calls']) % 2 == 0
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    user_names, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    num = {n: i for i, n in enumerate(item_names) if n is not None}
    a = [l.rstrip('\n').split('\t') for l in open(plain)]
    b = [l.rstrip('\n').split('\t') for l in open(div)]
    assert [x[0] for x in a] == [x[0] for x in b] == list(user_names)
    emb = kept['emb'].numpy()
    changed, ilds = 0, []
    for (u, items, scores), (_, got_items, got_scores) in zip(a, b):
        pid = np.zeros(pool, np.int32)
        ps = np.full(pool, -np.inf, np.float32)
        names = items.split(' ') if items else []
        pid[:len(names)] = [num[n] for n in names]
        ps[:len(names)] = [np.float32(s) for s in scores.split(' ')] if names else []
        ri, rs, ild, _, _ = MR.mmr_user(emb.astype(np.float64), pid, ps, lam, k)
        keep = ri != 0
        assert got_items == ' '.join(item_names[int(i)] for i in ri[keep]), u
        assert got_scores == ' '.join('%.9g' % float(np.float32(s)) for s in rs[keep]), u
        changed += got_items.split(' ') != names[:k]
        if keep.sum() >= 2:
            ilds.append((MR.mmr_user(emb.astype(np.float64), pid, ps, 1.0, k)[2], ild))
    assert changed > 0
    line = [l for l in seen if l.startswith('recommend_ild')]
    assert len(line) == 1 and line[0].endswith(f'{len(ilds)} of {len(user_names)} users'), line
    got = [float(x) for x in re.findall(r' (\d\.\d{5})', line[0])]
    np.testing.assert_allclose(got, np.mean(ilds, axis=0), atol=2e-5)
    assert any(l.startswith('diversify: mmr, lambda 0, pool 12') for l in seen)
