"""CPU side of the exclusion lists of any length (include/a4r_exclude.h: a4r_topk_items_excl): the C boundary of the export (header, the
binding's table in adapter4rec_amd/_lib_exclude.py, the built library, refusals in front of the first HIP call), the restatement
(tests/exclude_ref.py), the file readers, the flags in both parsers and their refusals, and recommend / write_recommendations / write_audience /
the image runner on the stand-in library."""
import ctypes
import glob
import logging
import os
import re

import numpy as np
import pytest
import torch

import exclude_ref as XR
import sim_lib
from topk_ref import sim_topk_items, topk_reference

NAMES = ['a4r_topk_items_excl']
HEADER = ('include', 'a4r_exclude.h')


# ------------------------------------------------------------------ the C boundary, held as tests/test_audience_cpu.py holds its header
def exclude_prototypes():
    import test_abi_cpu as ABI
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', ABI.header(HEADER)):
        params = []
        for a in args.split(','):
            words = re.sub(r'/\*.*?\*/', ' ', re.sub(r'\bconst\b', ' ', a)).replace('*', ' * ').split()
            params.append((words[0], '*' in words))
        assert name not in out, name
        out[name] = (ret, params)
    return out


def test_signature_table_matches_the_header_and_the_library():
    import test_abi_cpu as ABI
    from adapter4rec_amd import _lib as L
    protos = exclude_prototypes()
    table = L.EXCLUDE_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    others = [t for m, (t, _) in L.SATELLITES.items() if m != '_lib_exclude']
    assert '_lib_exclude' in L.SATELLITES and len(others) == len(L.SATELLITES) - 1
    assert not set(table) & set(L.SIGNATURES).union(*(set(getattr(L, t)) for t in others))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I = ctypes.c_void_p, ctypes.c_int
    assert table['a4r_topk_items_excl'] == (_I, (_P,) * 9 + (_I,) * 4)
    assert [p for p in protos['a4r_topk_items_excl'][1]][3:6] == [('int64_t', True), ('int32_t', True), ('uint8_t', True)]      # excl_ptr, excl_idx, cand
    txt = ABI.header(HEADER)
    assert not re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt) and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    for phrase in ('no cap on a list', 'ascending\n *              within a user', 'match nothing', 'never reads outside', 'ties to the smaller id',
                   'does not depend on the grid', 'no float atomics', 'a4r_topk_ws_bytes(U, N1, K)', 'before\n * any HIP call', 'NaN sorts below -inf'):
        assert phrase in raw, phrase                                               # the rule is written down
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert a4r_h.count('#include "a4r_exclude.h"') == 1
    assert a4r_h.index('#include "a4r_audience.h"') < a4r_h.index('#include "a4r_exclude.h"')
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411      # no existing argument list changed
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_topk_items_excl(*([None] * 9), 'U', 2, 64, 1)
    mk = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'Makefile')).read()
    assert mk.count('../../include/a4r_exclude.h') == 3                            # the header in the three dependency lists
    src = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'a4r_topk.hip')).read()
    assert 'topk_excl_partial_kernel' in src and 'extern "C" int a4r_topk_items_excl' in src      # a sibling of topk_partial_kernel, in its file


def test_wrapper_is_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_exclude as B
    assert L.topk_items_excl is B.topk_items_excl and L.EXCLUDE_SIGNATURES is B.EXCLUDE_SIGNATURES


def test_export_refuses_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (nothing is enqueued, no GPU is needed): each required pointer in turn NULL (cand may be NULL:
    every probe runs with and without it), E not served, K outside 1 .. 256, U < 1, N1 < 2, a table off a 16-byte boundary, ws or excl_ptr off
    an 8-byte boundary."""
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    f = lib.a4r_topk_items_excl
    f.restype, f.argtypes = L.EXCLUDE_SIGNATURES['a4r_topk_items_excl']
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    # (stream, prec, item_emb, excl_ptr, excl_idx, cand, ids, scores, ws, U, N1, E, K)
    good = [None, p, p, p, p, p, p, p, p, 4, 100, 64, 10]
    probed = 0

    def refused(i, v):
        for cand in (p, None):
            a = list(good)
            a[5] = cand
            a[i] = v
            assert f(*a) == -1, (i, v, cand)
        return 1
    for i in (1, 2, 3, 4, 6, 7, 8):
        probed += refused(i, None)
    bad = [(11, 0), (11, 32), (11, 96), (11, 1024), (11, -64), (12, 0), (12, -1), (12, 257), (9, 0), (9, -1), (10, 1), (10, 0), (10, -5),
           (1, p + 4), (1, p + 8), (2, p + 4), (2, p + 12), (8, p + 4), (8, p + 1), (3, p + 4), (3, p + 2), (3, p + 12)]
    for i, v in bad:
        probed += refused(i, v)
    assert f(*([None] * 9), 0, 0, 0, 0) == -1
    assert probed == 7 + len(bad)


def test_wrapper_refuses_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, U, E, k = 9, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(prec=torch.zeros(U, E), item_emb=torch.zeros(N1, E), excl_ptr=torch.zeros(U + 1, dtype=torch.int64), excl_idx=i32(5), cand=None, k=k,
                ids=i32(U, k), scores=torch.zeros(U, k))
    call = lambda **kw: L.topk_items_excl(**dict(good, **kw))
    wide = torch.zeros(N1, 2 * E)[:, :E]
    off = lambda n: torch.zeros(n * E + 1)[1:].view(n, E)
    assert off(N1).data_ptr() % 16 == 4 and not wide.is_contiguous()
    for kw, msg in [(dict(item_emb=torch.zeros(N1, E, dtype=torch.float64)), 'contiguous fp32'), (dict(item_emb=wide), 'contiguous fp32'),
                    (dict(item_emb=off(N1)), '16-byte'), (dict(prec=off(U)), '16-byte'), (dict(prec=torch.zeros(U, 96), item_emb=torch.zeros(N1, 96)), 'E = 96'),
                    (dict(item_emb=torch.zeros(1, E)), 'N1 = 1'), (dict(item_emb=torch.zeros(N1 * E)), 'expected'), (dict(prec=torch.zeros(U, 128)), 'expected'),
                    (dict(prec=torch.zeros(U, E, dtype=torch.bfloat16)), 'contiguous fp32'),
                    (dict(excl_ptr=torch.zeros(U + 1, dtype=torch.int32)), 'excl_ptr must be contiguous int64'), (dict(excl_ptr=torch.zeros(U, dtype=torch.int64)), 'excl_ptr'),
                    (dict(excl_ptr=torch.zeros(2 * U + 2, dtype=torch.int64)[::2]), 'excl_ptr'), (dict(excl_ptr=torch.zeros(U + 1, 1, dtype=torch.int64)), 'excl_ptr'),
                    (dict(excl_idx=i32(5).long()), 'excl_idx must be contiguous int32'), (dict(excl_idx=i32(5, 1)), 'excl_idx'), (dict(excl_idx=i32(10)[::2]), 'excl_idx'),
                    (dict(cand=torch.ones(N1 + 1, dtype=torch.uint8)), 'cand'), (dict(cand=torch.ones(N1, dtype=torch.int32)), 'cand'),
                    (dict(cand=torch.ones(2 * N1, dtype=torch.uint8)[::2]), 'cand'), (dict(cand=torch.ones(N1, dtype=torch.uint8)), 'device tensor'),
                    (dict(cand=[1] * N1), 'cand'), (dict(k=0), 'k = 0'), (dict(k=257), 'k = 257'),
                    (dict(ids=i32(U, k + 1)), 'ids and scores'), (dict(ids=i32(U, k).long()), 'ids'), (dict(scores=torch.zeros(U + 1, k)), 'ids and scores'),
                    (dict(scores=torch.zeros(U, k, dtype=torch.float64)), 'scores')]:
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(RuntimeError, match='device tensors'):
        monkeypatch.undo()
        L.topk_items_excl(**good)                                                  # host tensors never reach a kernel


# ------------------------------------------------------------------ the restatement and the CSR builder
def test_restatement_and_csr():
    rng = np.random.default_rng(2)
    U, N1, k = 6, 40, 12
    s = rng.integers(-4, 5, size=(U, N1)).astype(np.float32)                       # many ties
    s[2, 7], s[2, 9] = np.nan, -0.0
    lists = [[], [3, 3, 0, -2, N1, N1 + 7, 5], list(range(1, N1)), list(range(4, N1)), rng.integers(1, N1, size=1000).tolist(), [1]]
    ri, rs = XR.excl_reference(s, lists, k)
    for u in range(U):                                                             # from the definition, pair by pair
        rows = sorted(((np.isnan(s[u, i]), -s[u, i] if not np.isnan(s[u, i]) else 0.0, i) for i in range(1, N1) if i not in lists[u]))[:k]
        want = [i for _, _, i in rows] + [0] * (k - len(rows))
        assert ri[u].tolist() == want, u
        assert np.isneginf(rs[u, len(rows):]).all()
    assert (ri[2] == 0).all() and ri[3, :3].tolist() == sorted([1, 2, 3], key=lambda i: (-s[3, i], i)) and (ri[3, 3:] == 0).all()
    short, _ = topk_reference(s, [l[:264] for l in lists], k)                      # on lists a4r_topk_items serves: its restatement's lists
    for u in (0, 1, 5):
        assert ri[u].tolist() == short[u].tolist()
    cand = (rng.random(N1) < 0.4)
    ci, _ = XR.excl_reference(s, lists, k, cand)
    for u in range(U):
        keep = [i for i in XR.excl_reference(s[u:u + 1], [lists[u]], N1 - 1)[0][0] if i != 0 and cand[i]]
        assert ci[u].tolist() == (keep + [0] * k)[:k], u
    ptr, flat = XR.csr64(lists)
    assert ptr.dtype == np.int64 and flat.dtype == np.int32 and ptr.tolist() == np.concatenate([[0], np.cumsum([len(l) for l in lists])]).tolist()
    assert flat.size == ptr[-1] + 1 and flat[-1] == 0
    for u in range(U):
        row = flat[ptr[u]:ptr[u + 1]]
        assert row.tolist() == sorted(lists[u])                                    # ascending, repeats and ids that are no item kept
    out_i, out_s = torch.zeros(U, k, dtype=torch.int32), torch.zeros(U, k)
    prec, emb = torch.from_numpy(np.eye(U, 64, dtype=np.float32)), torch.zeros(N1, 64)
    emb[:, :U] = torch.from_numpy(np.nan_to_num(s).T.copy())
    XR.sim_topk_items_excl(prec, emb, torch.from_numpy(ptr), torch.from_numpy(flat), None, k, out_i, out_s)
    wi, _ = XR.excl_reference(np.nan_to_num(s), lists, k)
    assert out_i.tolist() == wi.tolist()


# ------------------------------------------------------------------ the readers
def test_read_exclude_lists(tmp_path):
    from adapter4rec_amd.data_utils.metrics import read_exclude_lists
    users = ['ann', 'bob', 'cy']
    items = [None, 'A', 'B', 'C', 'D']
    f = tmp_path / 'x.tsv'
    f.write_text('ann\tA B A\n\nghost\tA\nbob\t\n  \nann\tD gone B gone\ncy\told\nghost\tB\nphantom\tA\n')
    lists, bad_users, bad_items = read_exclude_lists(str(f), users, items)
    assert lists == {0: [1, 2, 1, 4, 2], 1: [], 2: []}                             # duplicates kept (the union is made unique later); a user named twice: appended
    assert (bad_users, bad_items) == (2, 2)                                        # ghost, phantom; gone, old -- skipped and counted, each name once
    f.write_text('')
    assert read_exclude_lists(str(f), users, items) == ({}, 0, 0)


def test_read_full_histories(tmp_path):
    from adapter4rec_amd.data_utils.metrics import read_full_histories
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    name2id = {f'i{j}': j for j in range(1, 41)}
    f = tmp_path / 'b.tsv'
    long_line = [f'i{j}' for j in range(1, 31)]                                    # 30 items: the reader keeps the last 23, i8 .. i30
    f.write_text('u0\t' + ' '.join(long_line) + '\nu1\ti1 i2 i3\nu2\ti31 i9 i9 i32 i10 i33\n')
    user_names, item_names = read_behavior_names(str(f), name2id, 20, 5)
    assert user_names == ['u0', 'u2'] and 'i1' not in item_names and 'i8' in item_names
    lists, bad_users, bad_items = read_full_histories(str(f), name2id, user_names, item_names)
    idx = {n: i for i, n in enumerate(item_names) if n}
    assert lists[0] == [idx[f'i{j}'] for j in range(8, 31)]                        # i1 .. i7 occur only in the older part of the line and are in no
    assert (bad_users, bad_items) == (1, 7)                                        # window: no item of the catalogue -- skipped and counted; u1: too short
    assert lists[1] == [idx[n] for n in ('i31', 'i9', 'i9', 'i32', 'i10', 'i33')]
    # an item that occurs only in the older part of one line and inside another user's window: an id, beyond the first user's window
    f.write_text('u0\t' + ' '.join(['i40'] + long_line) + '\nu2\ti31 i9 i40 i32 i10 i33\n')
    user_names, item_names = read_behavior_names(str(f), name2id, 20, 5)
    idx = {n: i for i, n in enumerate(item_names) if n}
    lists, bad_users, bad_items = read_full_histories(str(f), name2id, user_names, item_names)
    assert lists[0][0] == idx['i40'] and len(lists[0]) == 24 and (bad_users, bad_items) == (0, 7)


def test_union_csr_is_sorted_unique_and_inside_the_table():
    from adapter4rec_amd.data_utils.metrics import exclude_union_csr, merge_exclude_lists
    base = {0: [5, 3, 5], 1: torch.LongTensor([7]), 2: np.array([2, 9])}
    more = {0: [9, 3, 0, -4, 10, 11, 2 ** 40], 2: set(range(1, 2000))}
    ptr, flat = exclude_union_csr(base, more, [2, 0, 1, 0], 10)
    assert ptr.dtype == np.int64 and flat.dtype == np.int32 and ptr.tolist() == [0, 9, 12, 13, 16] and flat.size == 17
    rows = [flat[ptr[r]:ptr[r + 1]].tolist() for r in range(4)]
    assert rows == [list(range(1, 10)), [3, 5, 9], [7], [3, 5, 9]]                 # ids outside 1 .. N dropped; no cap
    assert merge_exclude_lists(None, None) is None and merge_exclude_lists(None, {1: [2]}) == {1: [2]}
    assert merge_exclude_lists({1: [2], 3: [4]}, {1: (5, 2)}) == {1: [2, 5, 2], 3: [4]}


# ------------------------------------------------------------------ the flags
def test_both_parsers_take_the_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert (a.exclude_lists, a.exclude_history) == (None, 'window')
        for mode in ('recommend', 'audience'):
            a = parse(['--mode', mode, '--exclude_lists', 'x.tsv', '--exclude_history', 'full'])
            assert (a.mode, a.exclude_lists, a.exclude_history) == (mode, 'x.tsv', 'full')
        with pytest.raises(SystemExit):
            parse(['--exclude_history', 'all'])


def test_flag_refusals():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    from adapter4rec_amd.data_utils.eval_flags import check_flags
    from adapter4rec_amd.parameters import parse_args
    both = (['--exclude_lists', 'x.tsv'], '--exclude_lists'), (['--exclude_history', 'full'], '--exclude_history full')
    for main in (run.main, run_adapter.main):
        for flags, name in both:
            for mode in ('train', 'test', 'similar'):
                with pytest.raises(ValueError, match=f'{name} is honoured by --mode recommend and --mode audience only, not by --mode {mode}'):
                    main(['--mode', mode] + flags)
            with pytest.raises(ValueError, match=f'{name} and --candidate_lists cannot be combined: a shortlist is filtered where it is made'):
                main(['--mode', 'recommend', '--candidate_lists', 'l.tsv'] + flags)
            with pytest.raises(ValueError, match=f'{name} and --score_dtype bf16 cannot be combined: a4r_topk_items_excl scores in fp32 only'):
                main(['--mode', 'recommend', '--score_dtype', 'bf16'] + flags)
            # no existing message displaced: the checks in front keep their precedence
            with pytest.raises(ValueError, match='--score_dtype bf16 is not honoured by --mode audience'):
                main(['--mode', 'audience', '--score_dtype', 'bf16'] + flags)
            with pytest.raises(ValueError, match='--candidate_lists is honoured by --mode test and --mode recommend only, not by --mode audience'):
                main(['--mode', 'audience', '--candidate_lists', 'l.tsv'] + flags)
            with pytest.raises(ValueError, match='--candidate_lists is honoured by --mode test and --mode recommend only, not by --mode train'):
                main(['--mode', 'train', '--candidate_lists', 'l.tsv'] + flags)
            with pytest.raises(ValueError, match='--candidate_lists .a list per user. and --candidate_items'):
                main(['--mode', 'recommend', '--candidate_lists', 'l.tsv', '--candidate_items', 'c.txt'] + flags)
            with pytest.raises(ValueError, match='--score_dtype bf16 and --candidate_lists cannot be combined'):
                main(['--mode', 'recommend', '--candidate_lists', 'l.tsv', '--score_dtype', 'bf16'] + flags)
            with pytest.raises(ValueError, match='--score_dtype bf16 and --diversify mmr cannot be combined'):
                main(['--mode', 'recommend', '--diversify', 'mmr', '--score_dtype', 'bf16'] + flags)
            with pytest.raises(ValueError, match='--audience_out is honoured by --mode audience only, not by --mode recommend'):
                main(['--mode', 'recommend', '--audience_out', 'o.tsv'] + flags)
            with pytest.raises(ValueError, match='--eval_negatives is an evaluation protocol: it is not honoured by --mode recommend'):
                main(['--mode', 'recommend', '--eval_negatives', '10'] + flags)
    for argv in (['--mode', 'recommend', '--exclude_lists', 'x.tsv'], ['--mode', 'audience', '--exclude_history', 'full'],
                 ['--mode', 'recommend', '--exclude_lists', 'x.tsv', '--exclude_history', 'full', '--candidate_items', 'c.txt', '--diversify', 'mmr'],
                 ['--mode', 'audience', '--exclude_lists', 'x.tsv', '--exclude_history', 'full', '--audience_items', 'q.txt'],
                 ['--mode', 'train'], ['--mode', 'train', '--exclude_history', 'window'], ['--mode', 'recommend', '--score_dtype', 'bf16']):
        check_flags(parse_args(argv))                                              # what is honoured passes


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def _recording(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores):
    CALLS.append(dict(U=int(prec.shape[0]), k=int(k), cand=cand, ptr=excl_ptr, flat=excl_idx))
    return XR.sim_topk_items_excl(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores)


def _refuse(*a, **k):
    raise AssertionError('the exclusion-list entry called without exclude_lists')


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


@pytest.fixture
def simulated(monkeypatch):
    import mmr_ref as MR
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    from test_candidates_cpu import sim_topk_items_cand
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'mmr_rerank', MR.sim_mmr_rerank, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_excl', _recording, raising=False)
    CALLS.clear()


def _long_lists(rng, item_num, users):
    """1 000 ids each, far beyond the 264-id cap: repeats and ids that are no item among them, about a third of the catalogue left"""
    out = {}
    for u in users:
        blocked = rng.choice(np.arange(1, item_num + 1), size=(2 * item_num) // 3, replace=False)
        out[u] = np.concatenate([rng.choice(blocked, size=990), [0, -3, item_num + 1, item_num + 9, 2 ** 40], blocked[:5]]).tolist()
        assert len(out[u]) == 1000
    return out


def test_recommend_excludes_the_union(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(13)
    n, k = len(eval_seq), 6
    rng = np.random.default_rng(1)
    lists = _long_lists(rng, item_num, range(0, n, 2))
    lists[1] = []
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '5')
    plain_i, plain_s = recommend(model, eval_seq, emb, k, args)
    assert CALLS == []                                                             # without the keyword: the entry it called before
    ids, sc = recommend(model, eval_seq, emb, k, args, exclude_lists=lists)
    assert [c['U'] for c in CALLS] == [5, 5, 3] and all(c['cand'] is None and c['k'] == k for c in CALLS)
    assert all(c['flat'] is CALLS[0]['flat'] for c in CALLS) and CALLS[0]['ptr'].dtype == torch.int64 and CALLS[0]['flat'].dtype == torch.int32
    assert CALLS[1]['ptr'].data_ptr() == CALLS[0]['ptr'].data_ptr() + 5 * 8        # uploaded once, sliced per batch
    flat = CALLS[0]['flat'].numpy()
    p = np.concatenate([c['ptr'].numpy()[:-1] for c in CALLS] + [CALLS[-1]['ptr'].numpy()[-1:]])
    for u in range(n):
        union = sorted({i for i in lists.get(u, []) if 1 <= i <= item_num} | set(eval_seq[u]))      # the window list and the long one
        assert flat[p[u]:p[u + 1]].tolist() == union, u
        got = set(ids[u].tolist()) - {0}
        assert not got & set(union) and len(got) == min(k, item_num - len(union)), u
        if u % 2:
            assert torch.equal(ids[u], plain_i[u]) and torch.equal(sc[u], plain_s[u])      # no list, or an empty one: the plain call's list
    with pytest.raises(ValueError, match='exclusion list of 1000 items exceeds'):   # the same 1 000-id lists through exclude=: the cap
        recommend(model, eval_seq, emb, k, args, exclude={u: lists.get(u, [1]) for u in range(n)})
    want_i, want_s = XR.excl_reference((CALLS_PREC(model, eval_seq, emb, args) @ emb.t()).numpy(), [flat[p[u]:p[u + 1]] for u in range(n)], k)
    assert ids.tolist() == want_i.tolist()
    # exclude= and exclude_lists= together: their union, and no cap on exclude= either
    CALLS.clear()
    excl = {u: list(range(1, 301)) if u == 2 else [1] for u in range(n)}
    ids, _ = recommend(model, eval_seq, emb, k, args, exclude=excl, exclude_lists={3: [2, 2, 5]})
    rows = np.concatenate([c['ptr'].numpy()[:-1] for c in CALLS] + [CALLS[-1]['ptr'].numpy()[-1:]])
    f = CALLS[0]['flat'].numpy()
    assert f[rows[2]:rows[3]].tolist() == list(range(1, min(300, item_num) + 1)) and f[rows[3]:rows[4]].tolist() == [1, 2, 5] and f[rows[0]:rows[1]].tolist() == [1]
    # beside candidates: the mask goes to the same entry
    CALLS.clear()
    mask = np.zeros(item_num + 1, bool)
    mask[rng.choice(np.arange(1, item_num + 1), size=item_num // 2, replace=False)] = True
    ci, _ = recommend(model, eval_seq, emb, k, args, exclude_lists=lists, candidates=mask)
    assert len(CALLS) == 3 and all(c['cand'] is CALLS[0]['cand'] and c['cand'].dtype == torch.uint8 for c in CALLS) and CALLS[0]['cand'].tolist() == mask.astype(int).tolist()
    for u in range(n):
        got = set(ci[u].tolist()) - {0}
        assert mask[sorted(got)].all() and not got & (set(lists.get(u, [])) | set(eval_seq[u])), u
    # beside diversify: the pool is the new entry's output at K = pool
    CALLS.clear()
    di, _ = recommend(model, eval_seq, emb, 3, args, exclude_lists=lists, diversify=Diversify(0.5, 9))
    assert [c['k'] for c in CALLS] == [9, 9, 9] and tuple(di.shape) == (n, 3)
    pool, _ = recommend(model, eval_seq, emb, 9, args, exclude_lists=lists)
    for u in range(n):
        assert set(di[u].tolist()) - {0} <= set(pool[u].tolist()) - {0} and not set(di[u].tolist()) & set(lists.get(u, [])) - {0}, u
    # refused before anything is encoded
    monkeypatch.setattr(model, 'eval', lambda: pytest.fail('a refused call reached the model'))
    with pytest.raises(ValueError, match='exclude_lists cannot be combined with candidate_lists: a shortlist is filtered where it is made'):
        recommend(model, eval_seq, emb, k, args, exclude_lists=lists, candidate_lists={0: [1, 2]})
    with pytest.raises(ValueError, match="exclude_lists cannot be combined with score_dtype 'bf16'"):
        recommend(model, eval_seq, emb, k, args, exclude_lists=lists, score_dtype='bf16')
    with pytest.raises(ValueError, match='a dict'):
        recommend(model, eval_seq, emb, k, args, exclude_lists=[[1], [2]])


def CALLS_PREC(model, eval_seq, emb, args):
    from adapter4rec_amd.data_utils.metrics import user_vectors
    return user_vectors(model, eval_seq, emb, args)


def test_without_the_keyword_nothing_changes(simulated, monkeypatch, tmp_path):
    """recommend and write_recommendations make exactly the calls they made before, and exclude= alone still raises at 265 ids"""
    from test_candidates_cpu import _id_model_and_users, sim_topk_items_cand
    from adapter4rec_amd.data_utils.metrics import recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(12)
    monkeypatch.setattr(sim_lib, 'topk_items_excl', _refuse)
    seen = []

    def keep(name, fn):
        def f(*a):
            seen.append((name, tuple(a[2].shape), a[2].dtype))                     # the offsets: int32, counted from the batch's first id
            return fn(*a)
        return f
    monkeypatch.setattr(sim_lib, 'topk_items', keep('topk_items', sim_topk_items))
    monkeypatch.setattr(sim_lib, 'topk_items_cand', keep('topk_items_cand', sim_topk_items_cand))
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '8')
    recommend(model, eval_seq, emb, 5, args)
    mask = np.ones(item_num + 1, bool)
    recommend(model, eval_seq, emb, 5, args, candidates=mask)
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    write_recommendations(model, eval_seq, hist, emb, 5, 16, args, [f'U{u}' for u in eval_seq], names, str(tmp_path / 'r.tsv'), Log_file=_Log())
    assert seen == [('topk_items', (9,), torch.int32), ('topk_items', (5,), torch.int32), ('topk_items_cand', (9,), torch.int32),
                    ('topk_items_cand', (5,), torch.int32), ('topk_items', (9,), torch.int32), ('topk_items', (9,), torch.int32)]       # (the writer pads its shard to the batch size: 16 users)
    with pytest.raises(ValueError, match='exclusion list of 265 items exceeds A4R_EVAL_MAX_HISTORY = 264'):
        recommend(model, eval_seq, emb, 5, args, exclude={u: list(range(1, 266)) for u in eval_seq})
    with pytest.raises(AssertionError, match='without exclude_lists'):
        recommend(model, eval_seq, emb, 5, args, exclude_lists={})                 # the keyword given, even empty: every batch through the new entry


def test_write_recommendations_excludes_the_union(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(20)
    n, k = len(eval_seq), 4
    rng = np.random.default_rng(3)
    lists = _long_lists(rng, item_num, range(0, n, 3))
    user_names = [f'U{u:02d}' for u in range(n)]
    item_names = [None] + [f'I{i:03d}' for i in range(1, item_num + 1)]
    path = str(tmp_path / 'rec.tsv')
    assert write_recommendations(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, Log_file=_Log(), exclude_lists=lists) == path
    assert len(CALLS) >= 1 and sum(c['U'] for c in CALLS) >= n
    window = {u: np.concatenate([np.asarray(hist[u]), np.asarray(eval_seq[u][-1:])]) for u in range(n)}
    ids, sc = recommend(model, eval_seq, emb, k, args, exclude=window, exclude_lists=lists)
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    assert [r[0] for r in rows] == user_names
    for u, r in enumerate(rows):
        keep = ids[u] != 0
        assert r[1].split(' ') == [item_names[int(i)] for i in ids[u][keep]] and r[2].split(' ') == ['%.9g' % float(s) for s in sc[u][keep]]
        blocked = {item_names[i] for i in lists.get(u, []) if 1 <= i <= item_num} | {item_names[int(i)] for i in window[u]}
        assert not set(r[1].split(' ')) & blocked, u
    # beside candidates and diversify, in one call
    CALLS.clear()
    mask = np.zeros(item_num + 1, bool)
    mask[1::2] = True
    log = _Log()
    write_recommendations(model, eval_seq, hist, emb, 3, 16, args, user_names, item_names, path, candidates=mask, diversify=Diversify(0.6, 8), Log_file=log,
                          exclude_lists=lists)
    assert all(c['k'] == 8 and c['cand'] is not None for c in CALLS) and len(log.lines) == 1 and log.lines[0].startswith('recommend_ild')
    for u, l in enumerate(open(path)):
        items = l.rstrip('\n').split('\t')[1].split()
        assert len(items) <= 3 and all(mask[item_names.index(x)] for x in items)
        assert not set(items) & ({item_names[i] for i in lists.get(u, []) if 1 <= i <= item_num} | {item_names[int(i)] for i in window[u]}), u


def test_write_audience_merges_the_lists_into_the_seen_lists(simulated, monkeypatch, tmp_path):
    import audience_ref as AR
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import audience_seen_csr, write_audience
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(18)
    n, k = len(eval_seq), 5
    got = []

    def keeping(item_emb, query, user_vec, seen_ptr, seen_idx, elig, kk, rows, scores):
        got.append((seen_ptr.clone(), seen_idx.clone()))
        return AR.sim_topk_users(item_emb, query, user_vec, seen_ptr, seen_idx, elig, kk, rows, scores)
    monkeypatch.setattr(sim_lib, 'topk_users', keeping, raising=False)
    user_names = [f'U{u:02d}' for u in range(n)]
    item_names = [None] + [f'I{i:03d}' for i in range(1, item_num + 1)]
    rng = np.random.default_rng(4)
    lists = _long_lists(rng, item_num, [2, 7])
    lists[4] = list(range(1, item_num + 1))                                        # a user who may be shown nothing
    path = str(tmp_path / 'aud.tsv')
    write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, Log_file=_Log(), exclude_lists=lists)
    seen = [sorted(set(np.asarray(hist[u]).tolist()) | set(eval_seq[u][-1:]) | set(lists.get(u, []))) for u in range(n)]
    want_ptr, want_flat = audience_seen_csr(seen, n)
    assert got and got[0][0].tolist() == want_ptr.tolist() and got[0][1].tolist() == want_flat.tolist()
    by_item = {l.split('\t')[0]: l.rstrip('\n').split('\t')[1].split(' ') for l in open(path)}
    assert not any('U04' in us for us in by_item.values())
    for u in (2, 7):
        for i in lists[u]:
            if 1 <= i <= item_num:
                assert user_names[u] not in by_item.get(item_names[i], []), (u, i)
    got.clear()
    write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, Log_file=_Log())      # without the keyword: the seen lists as they were
    plain = [np.concatenate([np.asarray(hist[u]), np.asarray(eval_seq[u][-1:])]) for u in range(n)]
    assert got[0][1].tolist() == audience_seen_csr(plain, n)[1].tolist()
    assert CALLS == []                                                             # Python only: the item-side entry is not involved


# ------------------------------------------------------------------ the entry point
def test_cv_id_runner_exclude_flags(tmp_path, monkeypatch):
    """the image entry point with --item_tower id on the stand-in library: train one epoch, then --mode recommend --exclude_history full
    --exclude_lists f.tsv: every line against the stand-in on the union, the log line's counts; then --mode audience with the same flags"""
    import audience_ref as AR
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.data_utils import read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    for name in ('id_index', 'id_grad_sum', 'id_index_ws_ints'):
        if hasattr(IC, name):
            monkeypatch.setattr(sim_lib, name, getattr(IC, name), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_excl', _refuse, raising=False)
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))      # training and its evaluation never call the new entry
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    seen_lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen_lines.append(record.getMessage())
    orig_setup = RA.setuplogger

    def setup(*a, **kw):                                                          # (_run_cv drops the loggers' handlers after every run)
        out = orig_setup(*a, **kw)
        logging.getLogger('Log_file').addHandler(Keep())
        return out
    monkeypatch.setattr(RA, 'setuplogger', setup)
    rec = dict(loss=[], batch=[], eval=[])
    plain = os.path.join(root, 'plain.tsv')
    CR._run_cv(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--recommend_out', plain], monkeypatch, rec)
    assert not [l for l in seen_lines if l.startswith('exclude lists')]            # without the flags: the old entry, no log line
    behaviours = os.path.join(data, 'toy', 'users_log.tsv')
    _, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    user_names, item_names = read_behavior_names(behaviours, name2id, 20, 5)
    known = set(item_names[1:])
    full = {l.split('\t')[0]: set(l.rstrip('\n').split('\t')[1].split(' ')) for l in open(behaviours)}
    assert any(len(v) > 23 for v in full.values())
    first = {l.split('\t')[0]: l.rstrip('\n').split('\t')[1].split(' ') for l in open(plain)}
    blocked = {u: first[u][:2] for u in user_names[::2]}
    f = os.path.join(root, 'f.tsv')
    with open(f, 'w') as fh:
        for u, items in blocked.items():
            fh.write(u + '\t' + ' '.join(items + ['gone_item']) + '\n')
        fh.write('nobody\tv1 v2\n\n')
    CALLS.clear()
    monkeypatch.setattr(sim_lib, 'topk_items_excl', _recording)
    monkeypatch.setattr(sim_lib, 'topk_items', lambda *a: pytest.fail('the capped entry called under --exclude_lists'))
    out = os.path.join(root, 'rec.tsv')
    CR._run_cv(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--recommend_out', out, '--exclude_history', 'full',
                         '--exclude_lists', f], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == [] and len(CALLS) >= 1
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert [r[0] for r in rows] == user_names
    want = {u: (full[u] & known) | set(blocked.get(u, ())) for u in user_names}
    flat = CALLS[0]['flat'].numpy()
    p = np.concatenate([c['ptr'].numpy()[:-1] for c in CALLS] + [CALLS[-1]['ptr'].numpy()[-1:]])
    for u, (name, items, scores) in enumerate(rows):
        items = items.split(' ')
        assert len(items) == 5 and not set(items) & want[name], name
        assert {item_names[i] for i in flat[p[u]:p[u + 1]]} == want[name], name    # the union reached the kernel: the whole line, not its window
    assert sum(first[u] != r[1].split(' ') for u, r in zip(user_names, rows)) >= len(blocked)
    line = [l for l in seen_lines if l.startswith('exclude lists: ')]
    old = set().union(*full.values()) - known
    assert len(line) == 1 and line[0] == (f'exclude lists: {len(user_names)} users, {sum(len(v) for v in want.values())} ids in all, longest '
                                          f'{max(len(v) for v in want.values())}; 1 user names and {len(old) + 1} item names unknown, skipped <- '
                                          f'{behaviours} (--exclude_history full) + {f}')
    # --mode audience with the same flags: merged into the seen lists
    got = []

    def keeping(item_emb, query, user_vec, seen_ptr, seen_idx, elig, kk, rr, ss):
        got.append((seen_ptr.clone(), seen_idx.clone()))
        return AR.sim_topk_users(item_emb, query, user_vec, seen_ptr, seen_idx, elig, kk, rr, ss)
    monkeypatch.setattr(sim_lib, 'topk_users', keeping, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_excl', _refuse)
    CR._run_cv(common + ['--mode', 'audience', '--load_ckpt_name', 'epoch-1.pt', '--topk', '3', '--exclude_history', 'full', '--exclude_lists', f], monkeypatch, rec)
    sp, sf = got[0][0].numpy(), got[0][1].numpy()
    for u, name in enumerate(user_names):
        assert {item_names[i] for i in sf[sp[u + 1]:sp[u + 2]]} == want[name], name
    assert len([l for l in seen_lines if l.startswith('exclude lists: ')]) == 2
