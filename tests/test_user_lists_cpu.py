"""CPU side of per-user candidate lists (include/a4r_user_lists.h: a4r_topk_lists, a4r_eval_rank_lists): the C boundary of the two exports (header,
the binding's table in adapter4rec_amd/_lib_user_lists.py, the built library, refusals in front of the first HIP call), the wrappers' argument
checks, read_candidate_lists, --candidate_lists in both parsers and its refusals, eval_ranks / eval_model / recommend / write_recommendations
with lists on simulated kernels against the numpy restatement (tests/lists_ref.py), the text runner's --mode recommend --candidate_lists file,
and the gap-rule cap of the random case of tests/test_user_lists_gpu.py."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import lists_ref as LR
import sim_lib
from topk_ref import sim_topk_items

NAMES = ['a4r_eval_rank_lists', 'a4r_topk_lists']
HEADER = ('include', 'a4r_user_lists.h')


# ------------------------------------------------------------------ the C boundary, held as tests/test_candidates_cpu.py holds its header
def list_prototypes():
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
    protos = list_prototypes()
    table = L.USER_LISTS_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    assert not set(table) & (set(L.SIGNATURES) | set(L.SCORE_CE_BF16_SIGNATURES) | set(L.CANDIDATES_SIGNATURES))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I = ctypes.c_void_p, ctypes.c_int
    assert table['a4r_topk_lists'] == (_I, (_P,) * 9 + (_I,) * 5) and table['a4r_eval_rank_lists'] == (_I, (_P,) * 9 + (_I,) * 4)
    txt = ABI.header(HEADER)
    defines = dict(re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt))
    assert defines == {'A4R_LIST_MAX': '4096'} and L.LIST_MAX == 4096 and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    assert 'NOT promised' in raw and 'MFMA' in raw                                # the score is not promised to be the sweep's bits, and says so
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert '#include "a4r_user_lists.h"' in a4r_h and '#include "a4r_candidates.h"' in a4r_h
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_topk_lists(*([None] * 9), 16.0, 100, 64, 10, 100)


def test_wrappers_are_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_user_lists as B
    assert L.topk_lists is B.topk_lists and L.eval_rank_lists is B.eval_rank_lists
    assert L.USER_LISTS_SIGNATURES is B.USER_LISTS_SIGNATURES and L.LIST_MAX == B.LIST_MAX == LR.LIST_MAX
    with pytest.raises(AttributeError):
        L.topk_user_lists


def _bound(name):
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    restype, argtypes = L.USER_LISTS_SIGNATURES[name]
    f = getattr(lib, name)
    f.argtypes, f.restype = argtypes, restype
    return f, sum(t is ctypes.c_void_p for t in argtypes)


def test_exports_refuse_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (so nothing is enqueued and no GPU is needed): every pointer NULL and every scalar 0; each
    pointer in turn NULL (the stream aside: NULL is the default stream) beside valid scalars and host addresses; then each scalar rule in turn
    -- U < 1, N1 < 2, E outside {64, 128, 256, 512}, K outside 1 .. 256, max_len outside 0 .. 4096 -- and misaligned prec / item_emb."""
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    probed = 0
    # scalars: topk (U, N1, E, K, max_len); rank (U, N1, E, max_len)
    for name, scalars, bad in (
            ('a4r_topk_lists', (16, 100, 64, 10, 100),
             [(0, 100, 64, 10, 100), (-1, 100, 64, 10, 100), (16, 1, 64, 10, 100), (16, 100, 96, 10, 100), (16, 100, 1024, 10, 100), (16, 100, 0, 10, 100),
              (16, 100, 64, 0, 100), (16, 100, 64, 257, 100), (16, 100, 64, 10, -1), (16, 100, 64, 10, 4097)]),
            ('a4r_eval_rank_lists', (16, 100, 64, 100),
             [(0, 100, 64, 100), (16, 1, 64, 100), (16, 100, 32, 100), (16, 100, 64, -1), (16, 100, 64, 4097)])):
        f, n_ptr = _bound(name)
        assert n_ptr + len(scalars) == len(f.argtypes)
        assert f(*([None] * n_ptr), *scalars) == -1, name
        assert f(*([None] * n_ptr), *([0] * len(scalars))) == -1, name
        for i in range(1, n_ptr):
            ptrs = [None] + [p16] * (n_ptr - 1)
            ptrs[i] = None
            assert f(*ptrs, *scalars) == -1, (name, i)
            probed += 1
        for sc in bad:
            assert f(None, *([p16] * (n_ptr - 1)), *sc) == -1, (name, sc)
        for which in (1, 2):                                                       # prec, item_emb off a 16-byte boundary
            ptrs = [None] + [p16] * (n_ptr - 1)
            ptrs[which] = p16 + 4
            assert f(*ptrs, *scalars) == -1, (name, which)
    assert probed == 8 + 8


# ------------------------------------------------------------------ the wrappers' checks
def test_wrappers_refuse_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, U, E, k = 9, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(prec=torch.zeros(U, E), item_emb=torch.zeros(N1, E), list_ptr=i32(U + 1), list_idx=i32(5), max_len=5, excl_ptr=i32(U + 1), excl_idx=i32(1),
                k=k, ids=i32(U, k), scores=torch.zeros(U, k))
    good_r = dict(prec=torch.zeros(U, E), item_emb=torch.zeros(N1, E), target=i32(U), list_ptr=i32(U + 1), list_idx=i32(5), max_len=5, hist_ptr=i32(U + 1),
                  hist_idx=i32(1), rank=i32(U))
    topk = lambda **kw: L.topk_lists(**dict(good, **kw))
    rank = lambda **kw: L.eval_rank_lists(**dict(good_r, **kw))
    both = [(dict(prec=torch.zeros(U, E, dtype=torch.float64)), 'prec'), (dict(item_emb=torch.zeros(N1, E, dtype=torch.bfloat16)), 'item_emb'),
            (dict(item_emb=torch.zeros(N1, 128)), 'expected'), (dict(prec=torch.zeros(U, 2 * E)[:, ::2]), 'prec'),
            (dict(prec=torch.zeros(U, 96), item_emb=torch.zeros(N1, 96)), 'E = 96'), (dict(item_emb=torch.zeros(1, E)), 'N1 = 1'),
            (dict(list_ptr=i32(U + 1).long()), 'list_ptr'), (dict(list_idx=i32(5).long()), 'list_idx'), (dict(list_idx=i32(10)[::2]), 'list_idx'),
            (dict(list_ptr=i32(U)), 'list_ptr'), (dict(list_ptr=i32(U + 2)), 'list_ptr'),
            (dict(max_len=L.LIST_MAX + 1), 'max_len'), (dict(max_len=-1), 'max_len')]
    for kw, msg in both + [(dict(excl_ptr=i32(U)), 'excl_ptr'), (dict(excl_idx=torch.zeros(1)), 'excl_idx'), (dict(k=0), 'k = 0'), (dict(k=257), 'k = 257'),
                           (dict(ids=i32(U, k).long()), 'ids'), (dict(scores=torch.zeros(U, k, dtype=torch.float64)), 'scores'),
                           (dict(ids=i32(U, k + 1)), 'ids and scores'), (dict(scores=torch.zeros(U, 2 * k)[:, ::2]), 'scores')]:
        with pytest.raises(ValueError, match=msg):
            topk(**kw)
    for kw, msg in both + [(dict(hist_ptr=i32(U + 3)), 'hist_ptr'), (dict(hist_idx=torch.zeros(1)), 'hist_idx'), (dict(target=i32(U).long()), 'target'),
                           (dict(target=i32(U + 1)), 'target'), (dict(rank=i32(U, 1)), 'rank'), (dict(rank=torch.zeros(U)), 'rank')]:
        with pytest.raises(ValueError, match=msg):
            rank(**kw)
    # misaligned operands (a view 4 bytes into an allocation)
    base = torch.zeros(U * E + 4)
    off = base[1:1 + U * E].view(U, E) if base.data_ptr() % 16 == 0 else base[:U * E].view(U, E)
    if off.data_ptr() % 16:
        with pytest.raises(ValueError, match='16-byte'):
            topk(prec=off)


def test_wrappers_pass_empty_lists_as_one_zero(monkeypatch):
    """an empty list_idx / excl_idx has no data pointer: the library gets a one-element zero tensor, and max_len as the caller gave it"""
    from adapter4rec_amd import _lib as L
    seen = []

    class Lib:
        def a4r_topk_lists(self, *a):
            seen.append(a)
            return 0

        def a4r_eval_rank_lists(self, *a):
            seen.append(a)
            return 0
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)
    monkeypatch.setattr(L, 'lib', lambda: Lib())
    monkeypatch.setattr(L, '_stream', lambda: 0)
    U, N1, E, k = 3, 5, 64, 2
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    L.topk_lists(torch.zeros(U, E), torch.zeros(N1, E), i32(U + 1), i32(0), 0, i32(U + 1), i32(0), k, i32(U, k), torch.zeros(U, k))
    L.eval_rank_lists(torch.zeros(U, E), torch.zeros(N1, E), i32(U), i32(U + 1), i32(0), 7, i32(U + 1), i32(0), i32(U))
    t, r = seen
    assert t[4] and t[6] and t[-5:] == (U, N1, E, k, 0)                            # list_idx, excl_idx: real addresses
    assert r[5] and r[7] and r[-4:] == (U, N1, E, 7)


# ------------------------------------------------------------------ the file and the flags
def test_read_candidate_lists(tmp_path):
    from adapter4rec_amd.cv.data_utils import read_candidate_lists as cv_read
    from adapter4rec_amd.data_utils.metrics import read_candidate_lists
    assert cv_read is read_candidate_lists
    users = ['U0', 'U1', 'U2', 'U3']
    items = [None, 'N7', 'N3', 'N12', 'N5']
    p = tmp_path / 'l.txt'
    p.write_text('U1\tN3 N5 N3\n\nU3\tN12\n  \nU1\tN7\nU2\t\nU0\n')
    got = read_candidate_lists(str(p), users, items)
    assert got == {1: [2, 4, 2, 1], 3: [3], 2: [], 0: []}                          # a second line appends; repeats are kept (the kernel counts them once)
    # the round trip: what was written is what is read
    want = {0: [1, 2, 3], 2: [4], 3: []}
    p.write_text(''.join(users[u] + '\t' + ' '.join(items[i] for i in l) + '\n' for u, l in want.items()))
    assert read_candidate_lists(str(p), users, items) == want
    p.write_text('U1\tN3\nU9\tN3\nX1\tN5\nU9\tN5\nX2\t\nX3\t\nX4\t\nX5\t\n')
    with pytest.raises(ValueError, match=r'6 name\(s\) that are no user.*U9, X1, X2, X3, X4 \.\.\.'):
        read_candidate_lists(str(p), users, items)
    p.write_text('U1\tN3 N99 Y1\nU2\tN99 Y2 Y3 Y4 Y5\n')
    with pytest.raises(ValueError, match=r'6 name\(s\) that are no item.*N99, Y1, Y2, Y3, Y4 \.\.\.'):
        read_candidate_lists(str(p), users, items)
    p.write_text('U1\tNone\n')                                                     # the pad item has no name
    with pytest.raises(ValueError, match='None'):
        read_candidate_lists(str(p), users, items)
    p.write_text('\n')
    assert read_candidate_lists(str(p), users, items) == {}


def test_both_parsers_take_the_flag():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        assert parse([]).candidate_lists is None and parse(['--mode', 'test']).candidate_lists is None
        a = parse(['--mode', 'recommend', '--candidate_lists', 'shortlists.tsv'])
        assert a.candidate_lists == 'shortlists.tsv' and a.candidate_items is None


def test_flag_is_refused_under_mode_train_and_beside_candidate_items():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    for main in (run.main, run_adapter.main):
        with pytest.raises(ValueError, match='--candidate_lists'):
            main(['--mode', 'train', '--candidate_lists', 'l.tsv'])
        with pytest.raises(ValueError, match='--candidate_lists'):
            main(['--candidate_lists', 'l.tsv'])
        for mode in ('test', 'recommend'):
            with pytest.raises(ValueError, match='cannot be combined'):
                main(['--mode', mode, '--candidate_lists', 'l.tsv', '--candidate_items', 'stock.txt'])
    with pytest.raises(ValueError, match='--candidate_lists'):
        run.main(['--mode', 'load', '--candidate_lists', 'l.tsv'])                    # (the text runner's --mode load trains)


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def sim_topk_lists(prec, item_emb, list_ptr, list_idx, max_len, excl_ptr, excl_idx, k, ids, scores):
    assert list_ptr.dtype == torch.int32 and list_idx.dtype == torch.int32 and list_ptr.numel() == prec.shape[0] + 1 and int(list_ptr[0]) == 0
    assert list_idx.numel() >= int(list_ptr[-1]) and 0 <= max_len <= LR.LIST_MAX
    assert int((list_ptr[1:] - list_ptr[:-1]).max()) == max_len                    # the batch's longest list, from the host
    CALLS.append(('topk', prec.detach().clone(), None))
    return LR.sim_topk_lists(prec, item_emb, list_ptr, list_idx, max_len, excl_ptr, excl_idx, k, ids, scores)


def sim_eval_rank_lists(prec, item_emb, target, list_ptr, list_idx, max_len, hist_ptr, hist_idx, rank):
    assert list_ptr.dtype == torch.int32 and list_idx.dtype == torch.int32 and list_ptr.numel() == prec.shape[0] + 1 and int(list_ptr[0]) == 0
    assert int((list_ptr[1:] - list_ptr[:-1]).max()) == max_len
    CALLS.append(('rank', prec.detach().clone(), target.clone()))
    return LR.sim_eval_rank_lists(prec, item_emb, target, list_ptr, list_idx, max_len, hist_ptr, hist_idx, rank)


def _refuse(*a, **k):
    raise AssertionError('a whole-table or candidate-set call under candidate lists / a lists call without them')


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_lists', sim_topk_lists, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', sim_eval_rank_lists, raising=False)
    CALLS.clear()


def _draw_lists(rng, users, item_num, eval_seq):
    """lists of 0 .. 60 ids with repeats, pad and out-of-range ids; every third holds the user's target"""
    out = {}
    for n, u in enumerate(users):
        x = rng.integers(-1, item_num + 3, size=int(rng.integers(0, 61)))
        if n % 3 == 0 and x.size:
            x[int(rng.integers(0, x.size))] = eval_seq[u][-1]
        out[u] = [int(v) for v in x]
    return out


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def test_eval_with_lists_against_the_restatement(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import eval_model, eval_ranks
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(24)
    U = len(eval_seq)
    target = np.array([eval_seq[u][-1] for u in range(U)])
    rng = np.random.default_rng(14)
    with_list = [u for u in range(U) if u % 4 != 1]                               # users 1, 5, 9, ... bring no list
    lists = _draw_lists(rng, with_list, item_num, eval_seq)
    lists[2] = []                                                                 # an empty list is a list: rank 1, counted
    hlists = [hist[u].numpy() for u in range(U)]
    assert any(set(lists[u]) & set(hlists[u].tolist()) for u in with_list)        # listed items the history takes out
    assert any(target[u] not in lists[u] for u in with_list)                      # targets that are not listed
    for name in ('eval_rank', 'eval_rank_cand', 'topk_items', 'topk_items_cand'):
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)               # under lists, no other entry is called
    ranks = eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidate_lists=lists).numpy()
    prec = torch.cat([c[1] for c in CALLS if c[0] == 'rank']).double().numpy()
    assert prec.shape[0] == U == len(ranks)                                       # a rank for every listed user, list or not
    s64 = prec @ emb.double().numpy().T
    full = [lists.get(u, []) for u in range(U)]
    want = LR.rank_lists_reference(s64, target, full, hlists)
    np.testing.assert_array_equal(ranks, want)
    assert all(ranks[u] == 1 for u in range(U) if u not in lists) and ranks[2] == 1 and (ranks > 1).any()
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', candidate_lists=lists)
    has = np.array([u in lists for u in range(U)])
    hit, ndcg, n = LR.hit_ndcg_means(want, has)
    assert n == len(lists) < U and abs(hr - hit) < 1e-7
    assert abs(hit - float((want <= 10).mean())) > 1e-3                           # the means leave the users without a list out
    line = [l for l in log.lines if 'test_results' in l][0]
    np.testing.assert_allclose([float(x) for x in line.split()[1:]], [hit * 100, ndcg * 100], atol=1e-4)
    assert [l for l in log.lines if l.startswith('test_candidate_lists')] == [f'test_candidate_lists   {n} of {U} users']
    # a sequence indexed by user id says the same as the mapping (None = no list)
    seq = [lists.get(u) for u in range(U)]
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidate_lists=seq) == hr
    # refusals: no user has a list, both restrictions, a list of 4097 ids (never truncated)
    with pytest.raises(ValueError, match='no user'):
        eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidate_lists={})
    with pytest.raises(ValueError, match='cannot be combined'):
        eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidate_lists=lists, candidates=np.ones(item_num + 1, bool))
    with pytest.raises(ValueError, match='cannot be combined'):
        eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidate_lists=lists, candidates=np.ones(item_num + 1, bool))
    long = dict(lists)
    long[7] = [1 + i % item_num for i in range(LR.LIST_MAX + 1)]
    with pytest.raises(ValueError, match=r'user 7: candidate list of 4097 items.*--candidate_items'):
        eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidate_lists=long)
    long[7] = long[7][:LR.LIST_MAX]                                               # 4096 is served
    assert eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidate_lists=long).shape == (U,)


def test_recommend_with_lists_against_the_restatement(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(37)
    U, k = len(eval_seq), 10
    rng = np.random.default_rng(15)
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    with_list = [u for u in range(U) if u % 5 != 2]
    lists = _draw_lists(rng, with_list, item_num, eval_seq)
    lists[0] = [2 ** 40, -2 ** 40, 3, 3, 2 ** 31]                                 # ids outside int32 are clamped to -1, not wrapped
    for name in ('eval_rank', 'eval_rank_cand', 'topk_items', 'topk_items_cand'):
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)
    ids, sc = recommend(model, seqs, emb, k, args, candidate_lists=lists)
    prec = torch.cat([c[1] for c in CALLS if c[0] == 'topk']).double().numpy()
    s64 = prec @ emb.double().numpy().T
    clean = {u: [v if -2 ** 31 <= v < 2 ** 31 else -1 for v in l] for u, l in lists.items()}
    ri, rs = LR.topk_lists_reference(s64, [clean.get(u, []) for u in range(U)], [seqs[u] for u in range(U)], k)
    np.testing.assert_array_equal(ids.numpy(), ri)
    np.testing.assert_allclose(sc.numpy(), rs, rtol=0, atol=1e-5 * np.abs(s64).max())
    got = ids.numpy()
    assert (got != 0).any() and got[0].tolist() == ([3] + [0] * (k - 1) if 3 not in seqs[0] else [0] * k)
    for u in range(U):
        assert set(got[u][got[u] != 0].tolist()) <= set(lists.get(u, [])) - set(seqs[u]), u
        assert len(set(got[u][got[u] != 0].tolist())) == int((got[u] != 0).sum()), u       # a repeated id is returned once
        if u not in lists:
            assert (got[u] == 0).all() and torch.isinf(sc[u]).all()
    # a subset of the users, in another order
    sub = [5, 0, 6]
    i2, _ = recommend(model, seqs, emb, k, args, candidate_lists=lists, user_ids=sub)
    np.testing.assert_array_equal(i2.numpy(), ri[sub])
    with pytest.raises(ValueError, match='cannot be combined'):
        recommend(model, seqs, emb, k, args, candidate_lists=lists, candidates=np.ones(item_num + 1, bool))
    with pytest.raises(ValueError, match=r'user 4: candidate list of 4097 items'):
        recommend(model, seqs, emb, k, args, candidate_lists={4: [1] * (LR.LIST_MAX + 1)})
    # the file: a line for every user with a list (an all-pad list gives an empty line), none for a user without
    user_names = [f'U{u}' for u in range(U)]
    item_names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    path = str(tmp_path / 'rec.tsv')
    assert write_recommendations(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, candidate_lists=lists) == path
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    assert [r[0] for r in rows] == [f'U{u}' for u in range(U) if u in lists]
    for name, items, scores in rows:
        u = int(name[1:])
        names = items.split(' ') if items else []
        assert set(int(x[1:]) for x in names) <= set(lists[u]) - set(eval_seq[u]) and len(scores.split(' ') if scores else []) == len(names)
    assert any(r[1] for r in rows)


def test_without_lists_the_lists_wrappers_are_never_called(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users, sim_eval_rank_cand, sim_topk_items_cand
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(20)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', _refuse)
    monkeypatch.setattr(sim_lib, 'topk_lists', _refuse)
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', sim_eval_rank_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand, raising=False)
    log = _Log()
    seqs = {u: eval_seq[u][:-1] for u in eval_seq}
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu')
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', candidate_lists=None) == hr
    assert not any('users' in l for l in log.lines)
    a = recommend(model, seqs, emb, 5, args)
    b = recommend(model, seqs, emb, 5, args, candidate_lists=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ones = np.ones(item_num + 1, bool)                                             # a candidate set still goes to the _cand entries
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=ones) == hr
    assert torch.equal(recommend(model, seqs, emb, 5, args, candidates=ones)[0], a[0])
    # every item listed for every user: the whole-table result (the stand-ins agree with each other)
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', sim_eval_rank_lists)
    monkeypatch.setattr(sim_lib, 'topk_lists', sim_topk_lists)
    everything = {u: range(1, item_num + 1) for u in eval_seq}
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidate_lists=everything) == hr
    assert torch.equal(recommend(model, seqs, emb, 5, args, candidate_lists=everything)[0], a[0])


def test_restatement_semantics():
    """the restatement itself: repeats count once, ids outside the table are ignored, max_len cuts the list, the target need not be listed, the
    exclusion list takes items out, lists keep topk_reference's order and padding"""
    s = np.array([[9.0, 1.0, 3.0, 3.0, 5.0, 2.0, 4.0]])
    i, v = LR.topk_lists_reference(s, [[3, 2, 3, 0, 7, -1, 5, 2]], [[]], 4)
    assert i.tolist() == [[2, 3, 5, 0]] and v[0, :3].tolist() == [3.0, 3.0, 2.0] and np.isinf(v[0, 3])
    assert LR.topk_lists_reference(s, [[3, 2, 3, 0, 7, -1, 5, 2]], [[2, 99, 0]], 4)[0].tolist() == [[3, 5, 0, 0]]
    assert LR.topk_lists_reference(s, [[5, 4, 6]], [[]], 2, max_len=2)[0].tolist() == [[4, 5]]
    assert LR.topk_lists_reference(s, [[5, 4, 6]], [[]], 2, max_len=0)[0].tolist() == [[0, 0]]
    assert LR.topk_lists_reference(s, [[]], [[1]], 2)[0].tolist() == [[0, 0]]
    assert LR.rank_lists_reference(s, [5], [[4, 4, 6, 1, 0, 9]], [[]]).tolist() == [3]          # 4 and 6 beat item 5; 4 counts once
    assert LR.rank_lists_reference(s, [5], [[4, 4, 6, 1]], [[6]]).tolist() == [2]
    assert LR.rank_lists_reference(s, [2], [[3, 2]], [[]]).tolist() == [1]                       # a tie does not beat the target
    assert LR.rank_lists_reference(s, [1], [[4, 6, 2]], [[]], max_len=1).tolist() == [2]
    assert LR.rank_lists_reference(s, [1], [[]], [[]]).tolist() == [1]
    ptr, flat = LR.csr_tail([[1, 2], [], [3]])
    assert ptr.tolist() == [0, 2, 2, 3] and flat.tolist() == [1, 2, 3] and ptr.dtype == flat.dtype == np.int32


@pytest.mark.parametrize('E', LR.RANDOM_E)
def test_random_case_is_decided_by_the_gap_rule(E):
    """The random-table case of tests/test_user_lists_gpu.py, from the fp64 reference alone: at least 95 % of the list positions that hold an item
    are separated from both neighbours by more than the fp32 summation bound, so the GPU test compares nearly every position."""
    prec, emb, lists, excl, target = LR.random_case(E)
    c = LR.RANDOM_CASE
    assert [len(l) for l in lists[:12]] == list(c['lengths']) and prec.shape == (48, E) and emb.shape == (4099, E)
    s64, bound, ri, rs, sure, real = LR.fp64_reference(prec, emb, lists, excl, c['K'])
    assert sure.shape == (c['U'], c['K']) and real.sum() > 300
    frac = sure.sum() / real.sum()
    print(f'E = {E}: {sure.sum()} of {real.sum()} item positions sure ({100 * frac:.1f} %)')
    assert frac >= 0.95, frac


# ------------------------------------------------------------------ the text entry point
def test_text_runner_recommend_with_candidate_lists(tmp_path, monkeypatch):
    """train one epoch through run.py, then --mode recommend --candidate_lists from its checkpoint: a line for every user of the file and no
    other, every recommended item from the user's own list and unseen, and the lines are the unrestricted run's with the unlisted items struck
    out."""
    import test_text_run as TR
    import test_topk_cpu as TC
    TC._simulated(monkeypatch)
    monkeypatch.setattr(sim_lib, 'topk_lists', sim_topk_lists, raising=False)
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'lists']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    user_names, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    names = item_names[1:]
    rng = np.random.default_rng(16)
    mine = {}
    lfile = os.path.join(root, 'shortlists.tsv')
    with open(lfile, 'w') as f:
        for n, u in enumerate(user_names):
            if n % 3 == 1:
                continue                                                          # a user without a list: no line in the output
            mine[u] = [str(x) for x in rng.choice(names, size=int(rng.integers(1, 25)))]          # (with repeats)
            half = len(mine[u]) // 2
            f.write(u + '\t' + ' '.join(mine[u][:half]) + '\n\n')
            f.write(u + '\t' + ' '.join(mine[u][half:]) + '\n')                   # the second line of a user is appended
    full, listed = os.path.join(root, 'full.tsv'), os.path.join(root, 'listed.tsv')
    rec = ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt']
    TR._run(common + rec + ['--recommend_out', full, '--topk', str(len(names))], monkeypatch, dict(loss=[], batch=[], eval=[]))
    monkeypatch.setattr(sim_lib, 'topk_items', _refuse)
    TR._run(common + rec + ['--recommend_out', listed, '--topk', '5', '--candidate_lists', lfile], monkeypatch, dict(loss=[], batch=[], eval=[]))
    a = {x[0]: x for x in (l.rstrip('\n').split('\t') for l in open(full))}
    b = [l.rstrip('\n').split('\t') for l in open(listed)]
    assert [x[0] for x in b] == [u for u in user_names if u in mine] and 0 < len(b) < len(a) == len(user_names)
    some = 0
    for u, items_b, scores_b in b:
        got = items_b.split(' ') if items_b else []
        want = [x for x in a[u][1].split(' ') if x in set(mine[u])][:5]
        assert got == want and len(scores_b.split(' ') if scores_b else []) == len(got), u
        some += len(got)
    assert some > 0
    # --mode test with the same file: both splits ranked within the users' own lists, `k of n users` beside each metrics line (TR._run's recorder
    # stands in for run_eval_once with the unrestricted argument list, so this run goes through run.main itself)
    import logging
    import socket
    import torch.distributed as dist
    from adapter4rec_amd import run
    monkeypatch.setattr(sim_lib, 'eval_rank_lists', sim_eval_rank_lists, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank', _refuse)
    CALLS.clear()
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    for k, v in dict(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='1', RANK='0', LOCAL_RANK='0').items():
        monkeypatch.setenv(k, v)
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    logging.getLogger('Log_file').addHandler(Keep())
    try:
        run.main(common + ['--mode', 'test', '--load_ckpt_name', 'epoch-1.pt', '--candidate_lists', lfile])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for name in ('Log_file', 'Log_screen'):
            lg = logging.getLogger(name)
            for h in list(lg.handlers):
                lg.removeHandler(h)
                h.close()
    assert any(l.startswith('candidate lists: %d of %d users' % (len(mine), len(user_names))) for l in seen), seen[-12:]
    for split in ('valid', 'test'):
        assert [l for l in seen if l.startswith(split + '_candidate_lists')] == ['%s_candidate_lists   %d of %d users' % (split, len(mine), len(user_names))]
    assert sum(c[0] == 'rank' for c in CALLS) >= 2
