"""CPU side of the audience lists (include/a4r_audience.h: a4r_topk_users): the C boundary of the export (header, the binding's table in
adapter4rec_amd/_lib_audience.py, the built library, refusals in front of the first HIP call), the rule on its restatement
(tests/audience_ref.py), the file readers, the CSR builder, the flags in both parsers and their refusals, and user_vectors / audience /
write_audience / the image runner on the stand-in library."""
import ctypes
import glob
import logging
import os
import re

import numpy as np
import pytest
import torch

import audience_ref as AR
import sim_lib

NAMES = ['a4r_topk_users']
HEADER = ('include', 'a4r_audience.h')


# ------------------------------------------------------------------ the C boundary, held as tests/test_similar_cpu.py holds its header
def audience_prototypes():
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
    protos = audience_prototypes()
    table = L.AUDIENCE_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    others = [t for m, (t, _) in L.SATELLITES.items() if m != '_lib_audience']
    assert '_lib_audience' in L.SATELLITES and len(others) == len(L.SATELLITES) - 1
    assert not set(table) & set(L.SIGNATURES).union(*(set(getattr(L, t)) for t in others))
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    _P, _I = ctypes.c_void_p, ctypes.c_int
    assert table['a4r_topk_users'] == (_I, (_P,) * 10 + (_I,) * 5)
    assert [p for p in protos['a4r_topk_users'][1]][4:7] == [('int64_t', True), ('int32_t', True), ('uint8_t', True)]      # seen_ptr, seen_idx, elig
    txt = ABI.header(HEADER)
    assert not re.findall(r'#define\s+(A4R_\w+)\s+(\d+)', txt) and 'typedef' not in txt
    raw = open(os.path.join(ABI.ROOT, *HEADER)).read()
    for phrase in ('whose seen list contains', 'ties to the smaller row', 'no item_emb row is read', 'does not depend on the grid', 'before\n * any HIP call',
                   'never reads outside', 'no cap on a list', 'a4r_topk_ws_bytes(Q, U1, K)'):
        assert phrase in raw, phrase                                               # the rule is written down
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert a4r_h.count('#include "a4r_audience.h"') == 1
    assert a4r_h.index('#include "a4r_similar.h"') < a4r_h.index('#include "a4r_audience.h"')
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411      # no existing argument list changed
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_topk_users(*([None] * 10), 'Q', 2, 2, 64, 1)
    mk = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'Makefile')).read()
    assert mk.count('../../include/a4r_audience.h') == 3                           # the header in the three dependency lists
    src = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'a4r_topk.hip')).read()
    assert 'audience_partial_kernel' in src and 'extern "C" int a4r_topk_users' in src       # a sibling of similar_partial_kernel, in its file


def test_wrapper_is_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_audience as B
    assert L.topk_users is B.topk_users and L.AUDIENCE_SIGNATURES is B.AUDIENCE_SIGNATURES


def test_export_refuses_bad_arguments_before_launching():
    """A4R_EINVAL in front of the first HIP call (nothing is enqueued, no GPU is needed): each required pointer in turn NULL (elig may be NULL:
    every probe runs with and without it), E not served, K outside 1 .. 256, Q < 1, N1 < 2, U1 < 2, a table off a 16-byte boundary, ws or
    seen_ptr off an 8-byte boundary."""
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    f = lib.a4r_topk_users
    f.restype, f.argtypes = L.AUDIENCE_SIGNATURES['a4r_topk_users']
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    # (stream, item_emb, query, user_vec, seen_ptr, seen_idx, elig, rows, scores, ws, Q, N1, U1, E, K)
    good = [None, p, p, p, p, p, p, p, p, p, 4, 100, 50, 64, 10]
    probed = 0

    def refused(i, v):
        for elig in (p, None):
            a = list(good)
            a[6] = elig
            a[i] = v
            assert f(*a) == -1, (i, v, elig)
        return 1
    for i in (1, 2, 3, 4, 5, 7, 8, 9):
        probed += refused(i, None)
    bad = [(13, 0), (13, 32), (13, 96), (13, 1024), (13, -64), (14, 0), (14, -1), (14, 257), (10, 0), (10, -1), (11, 1), (11, 0), (11, -5), (12, 1),
           (12, 0), (12, -7), (1, p + 4), (1, p + 8), (3, p + 4), (3, p + 12), (9, p + 4), (9, p + 1), (4, p + 4), (4, p + 2)]
    for i, v in bad:
        probed += refused(i, v)
    assert f(*([None] * 10), 0, 0, 0, 0, 0) == -1
    assert probed == 8 + len(bad)


def test_wrapper_refuses_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    monkeypatch.setattr(L, 'lib', lambda: pytest.fail('a refused call reached the library'))
    N1, U1, Q, E, k = 9, 7, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    good = dict(item_emb=torch.zeros(N1, E), query=i32(Q), user_vec=torch.zeros(U1, E), seen_ptr=torch.zeros(U1 + 1, dtype=torch.int64),
                seen_idx=i32(5), elig=torch.ones(U1, dtype=torch.uint8), k=k, rows=i32(Q, k), scores=torch.zeros(Q, k))
    call = lambda **kw: L.topk_users(**dict(good, **kw))
    wide = torch.zeros(N1, 2 * E)[:, :E]
    off = lambda n: torch.zeros(n * E + 1)[1:].view(n, E)
    assert off(N1).data_ptr() % 16 == 4 and not wide.is_contiguous()
    for kw, msg in [(dict(item_emb=torch.zeros(N1, E, dtype=torch.float64)), 'item_emb'), (dict(item_emb=wide), 'item_emb'), (dict(item_emb=off(N1)), 'item_emb must be 16-byte'),
                    (dict(item_emb=torch.zeros(N1, 96), user_vec=torch.zeros(U1, 96)), 'E = 96'), (dict(item_emb=torch.zeros(1, E)), 'N1 = 1'),
                    (dict(item_emb=torch.zeros(N1 * E)), 'expected'), (dict(user_vec=torch.zeros(U1, E, dtype=torch.float64)), 'user_vec'),
                    (dict(user_vec=off(U1)), 'user_vec must be 16-byte'), (dict(user_vec=torch.zeros(U1, 128)), 'expected'), (dict(user_vec=torch.zeros(U1 * E)), 'expected'),
                    (dict(user_vec=torch.zeros(1, E), seen_ptr=torch.zeros(2, dtype=torch.int64), elig=None), 'U1 = 1'),
                    (dict(query=i32(Q).long()), 'query'), (dict(query=i32(Q, 1)), 'query'), (dict(query=i32(2 * Q)[::2]), 'query'),
                    (dict(query=i32(0), rows=i32(0, k), scores=torch.zeros(0, k)), 'Q = 0'),
                    (dict(seen_ptr=torch.zeros(U1 + 1, dtype=torch.int32)), 'seen_ptr'), (dict(seen_ptr=torch.zeros(U1, dtype=torch.int64)), 'seen_ptr'),
                    (dict(seen_ptr=torch.zeros(2 * U1 + 2, dtype=torch.int64)[::2]), 'seen_ptr'), (dict(seen_idx=i32(5).long()), 'seen_idx'),
                    (dict(seen_idx=i32(5, 1)), 'seen_idx'), (dict(seen_idx=i32(10)[::2]), 'seen_idx'),
                    (dict(elig=torch.ones(U1 + 1, dtype=torch.uint8)), 'elig'), (dict(elig=torch.ones(U1, dtype=torch.int32)), 'elig'),
                    (dict(elig=torch.ones(2 * U1, dtype=torch.uint8)[::2]), 'elig'), (dict(k=0), 'k = 0'), (dict(k=257), 'k = 257'),
                    (dict(rows=i32(Q, k + 1)), 'ids and scores'), (dict(rows=i32(Q, k).long()), 'ids'), (dict(scores=torch.zeros(Q + 1, k)), 'ids and scores'),
                    (dict(scores=torch.zeros(Q, k, dtype=torch.float64)), 'scores')]:
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    with pytest.raises(RuntimeError, match='device tensors'):
        monkeypatch.undo()
        L.topk_users(**good)                                                       # host tensors never reach a kernel


# ------------------------------------------------------------------ the rule itself, on the restatement
def _brute(item, users, q, k, lists, elig):
    """one query, from the definition, pair by pair in Python floats"""
    if not 1 <= q < item.shape[0]:
        return [0] * k, [-np.inf] * k
    rows = []
    for r in range(1, users.shape[0]):
        if (elig is not None and not elig[r]) or q in list(lists[r]):
            continue
        rows.append((-float(np.dot(item[q].astype(np.float64), users[r].astype(np.float64))), r))
    rows.sort()
    return ([r for _, r in rows[:k]] + [0] * (k - min(k, len(rows))), [-s + 0.0 for s, _ in rows[:k]] + [-np.inf] * (k - min(k, len(rows))))


def test_restatement_against_the_definition():
    rng = np.random.default_rng(2)
    N1, U1, E = 12, 40, 64
    item, users = AR.integer_table(rng, N1, E), AR.integer_table(rng, U1, E)
    users[9], item[4] = users[3], 0                                                # equal rows: ties by row; a zero query: every score 0
    lists = [sorted(rng.choice(np.arange(1, N1), size=int(rng.integers(0, 6)), replace=False).tolist()) for _ in range(U1)]
    lists[5] = [3, 3, 3, 7, 40, -2]                                                # repeats, ids that are no item
    lists[0] = [1, 2, 3]                                                           # a list for the pad row
    ptr, flat = AR.csr(lists)
    elig = rng.random(U1) < 0.7
    query = [3, 7, 4, 0, -2, N1, 5, 5]
    for e in (None, elig):
        for k in (6, 64):
            ri, rs = AR.audience_reference(torch.from_numpy(item), torch.from_numpy(users), query, k, ptr, flat, e)
            for j, q in enumerate(query):
                bi, bs = _brute(item, users, q, k, lists, e)
                assert ri[j].tolist() == bi and rs[j].tolist() == bs, (k, q)
    ri, rs = AR.audience_reference(torch.from_numpy(item), torch.from_numpy(users), query, 64, ptr, flat)
    assert 5 not in ri[0] and 5 not in ri[1] and 0 not in ri[0, :20]               # row 5 has seen items 3 and 7; row 0 is never listed
    assert (ri[3:6] == 0).all() and np.isneginf(rs[3:6]).all() and (ri[6] == ri[7]).all()
    n = int((ri[2] != 0).sum())
    assert ri[2, :n].tolist() == sorted(ri[2, :n].tolist()) and (rs[2, :n] == 0).all() and not np.signbit(rs[2, :n]).any()      # all ties: by row; +0
    assert (ri[0, 39:] == 0).all() and np.isneginf(rs[0, 39:]).all()               # k beyond the table: pads


def test_stand_in_equals_the_restatement_on_integer_tables():
    rng = np.random.default_rng(3)
    N1, U1, E, k = 30, 70, 64, 9
    item, users = torch.from_numpy(AR.integer_table(rng, N1, E)), torch.from_numpy(AR.integer_table(rng, U1, E))
    ptr, flat = AR.csr_of_mask(rng.random((U1, N1)) < 0.2)
    elig = torch.from_numpy((rng.random(U1) < 0.5).astype(np.uint8))
    query = torch.tensor([1, 29, 30, 0, 7, 7], dtype=torch.int32)
    rows, sc = torch.zeros(6, k, dtype=torch.int32), torch.zeros(6, k)
    for e in (None, elig):
        AR.sim_topk_users(item, query, users, torch.from_numpy(ptr), torch.from_numpy(flat), e, k, rows, sc)
        ri, rs = AR.audience_reference(item, users, query, k, ptr, flat, e)
        np.testing.assert_array_equal(rows.numpy(), ri)
        np.testing.assert_array_equal(sc.numpy().astype(np.float64), rs)


@pytest.mark.parametrize('K,E,U1,Q,seed', AR.RANDOM_CASES)
def test_random_cases_are_decided_by_the_restatement_alone(K, E, U1, Q, seed):
    """The random cases of tests/test_audience_gpu.py from the restatement alone: 1.000 / 0.963 / 0.972 / 0.958 / 0.975 of the positions are
    decided (the GPU test's condition is 0.90), every list is full, and the 3 K best rows of the first query are not in its list."""
    item, users, query, mask = AR.random_case(K, E, U1, Q, seed)
    ptr, flat = AR.csr_of_mask(mask)
    ri, rs = AR.audience_reference(torch.from_numpy(item), torch.from_numpy(users), query, K + 1, ptr, flat)
    share = float(AR.decided(rs, AR.bounds(item, users, query).max(1)).mean())
    print(f'K = {K}, E = {E}, U1 = {U1}, Q = {Q}, seed {seed}: {share:.3f} of the positions decided')
    assert 0.90 <= share <= 1.0 and (ri != 0).all()
    plain = AR.audience_reference(torch.from_numpy(item), torch.from_numpy(users), query[:1], 3 * K, np.zeros(U1 + 1, np.int64), np.zeros(0, np.int32))[0]
    assert not set(plain[0]) & set(ri[0]) and mask[plain[0], query[0]].all()


# ------------------------------------------------------------------ the readers and the CSR builder
def test_read_audience_users_and_items(tmp_path):
    from adapter4rec_amd.data_utils.metrics import read_audience_users, read_similar_items
    users = [f'U{u}' for u in range(6)]
    f = tmp_path / 'u.txt'
    f.write_text('U4\n\n  U1 \nU4\n')
    m = read_audience_users(str(f), users)
    assert m.dtype == bool and m.tolist() == [False, True, False, False, True, False]
    f.write_text('U4\nnobody\nU9\nU9\n')
    with pytest.raises(ValueError, match='2 name.s. that are no user of this dataset: nobody, U9'):
        read_audience_users(str(f), users)
    f.write_text('\n'.join(f'x{i}' for i in range(7)) + '\n')
    with pytest.raises(ValueError, match=r'7 name.s. that are no user of this dataset: x0, x1, x2, x3, x4 \.\.\.'):
        read_audience_users(str(f), users)
    f.write_text('\n \n')
    with pytest.raises(ValueError, match='no user name'):
        read_audience_users(str(f), users)
    items = [None, 'A', 'B', 'C']
    f.write_text('C\nA\nC\n')
    assert read_similar_items(str(f), items).tolist() == [3, 1]                    # --audience_items: file order, read_similar_items reused


def test_seen_csr_is_sorted_unique_with_an_empty_row_0():
    from adapter4rec_amd.data_utils.metrics import audience_seen_csr
    seen = {0: [5, 3, 5, 9, 3], 1: [], 2: torch.LongTensor([7]), 3: np.array([2 ** 40, 4, -3, 4]), 4: list(range(1000, 0, -1))}
    ptr, flat = audience_seen_csr(seen, 5)
    assert ptr.dtype == np.int64 and flat.dtype == np.int32 and ptr.shape == (7,)
    rows = [flat[ptr[r]:ptr[r + 1]].tolist() for r in range(6)]
    assert rows[0] == [] and rows[1] == [3, 5, 9] and rows[2] == [] and rows[3] == [7] and rows[4] == [-1, 4]      # (ids below 0 or beyond int32: one -1)
    assert rows[5] == list(range(1, 1001))                                         # no cap on a list's length
    assert ptr[0] == 0 and ptr[-1] == flat.size and (np.diff(ptr) >= 0).all()
    ptr, flat = audience_seen_csr([[], []], 2)                                     # nothing seen at all: three empty rows
    assert ptr.tolist() == [0, 0, 0, 0] and flat.size == 0 and flat.dtype == np.int32


# ------------------------------------------------------------------ the flags
def test_both_parsers_take_the_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert (a.audience_out, a.audience_items, a.audience_users) == (None, None, None)
        a = parse(['--mode', 'audience', '--topk', '20', '--audience_out', 'o.tsv', '--audience_items', 'q.txt', '--audience_users', 'u.txt'])
        assert (a.mode, a.topk, a.audience_out, a.audience_items, a.audience_users) == ('audience', 20, 'o.tsv', 'q.txt', 'u.txt')
    with pytest.raises(SystemExit):
        parse_args(['--mode', 'crowd'])


def test_flag_refusals():
    """Before anything is set up (no device, no process group)."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    from adapter4rec_amd.data_utils.eval_flags import audience_out_path, check_flags
    from adapter4rec_amd.parameters import parse_args
    for main in (run.main, run_adapter.main):
        for mode in ('train', 'test', 'recommend', 'similar'):
            for flag in (['--audience_out', 'o.tsv'], ['--audience_items', 'q.txt'], ['--audience_users', 'u.txt']):
                with pytest.raises(ValueError, match=f'{flag[0]} is honoured by --mode audience only, not by --mode {mode}'):
                    main(['--mode', mode] + flag)
        for flags, msg in ((['--candidate_items', 'c.txt'], '--candidate_items'), (['--candidate_lists', 'l.tsv'], '--candidate_lists'),
                           (['--diversify', 'mmr'], '--diversify mmr'), (['--eval_negatives', '100'], '--eval_negatives'),
                           (['--eval_negatives_out', 'n.tsv'], '--eval_negatives'), (['--eval_neg_sampling', 'pop'], '--eval_neg_sampling'),
                           (['--eval_neg_seed', '7'], '--eval_neg_seed'), (['--similar_out', 's.tsv'], '--similar_out'),
                           (['--similar_items', 's.txt'], '--similar_items'), (['--similar_metric', 'dot'], '--similar_metric'),
                           (['--similar_min', '0.5'], '--similar_min'), (['--score_dtype', 'bf16'], '--score_dtype bf16 is not honoured by --mode audience')):
            with pytest.raises(ValueError, match=msg):
                main(['--mode', 'audience'] + flags)
    with pytest.raises(ValueError, match='--audience_users'):
        run.main(['--mode', 'load', '--audience_users', 'u.txt'])
    for argv in (['--mode', 'audience'], ['--mode', 'audience', '--audience_items', 'q.txt', '--audience_users', 'u.txt', '--audience_out', 'o.tsv', '--topk', '256'],
                 ['--mode', 'train'], ['--mode', 'similar', '--similar_metric', 'dot'], ['--mode', 'recommend', '--score_dtype', 'bf16']):
        check_flags(parse_args(argv))                                              # what is honoured passes
    a = parse_args(['--mode', 'audience', '--load_ckpt_name', 'epoch-3.pt'])
    assert audience_out_path(a, 'dir') == os.path.join('dir', 'audience_epoch-3.pt.tsv')
    a.audience_out = 'x.tsv'
    assert audience_out_path(a, 'dir') == 'x.tsv'


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def _recording(item_emb, query, user_vec, seen_ptr, seen_idx, elig, k, rows, scores):
    CALLS.append(dict(Q=int(query.numel()), elig=elig, k=int(k), emb=item_emb, table=user_vec, ptr=seen_ptr, flat=seen_idx))
    return AR.sim_topk_users(item_emb, query, user_vec, seen_ptr, seen_idx, elig, k, rows, scores)


def _refuse(*a, **k):
    raise AssertionError('the audience entry called under another mode')


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
    monkeypatch.setattr(sim_lib, 'topk_users', _recording, raising=False)
    CALLS.clear()


def _sim_lists(emb, table, query, k, seen, elig=None):
    """the stand-in's own lists for a user table and host-side seen lists -> (user ids = row - 1, scores) numpy"""
    from adapter4rec_amd.data_utils.metrics import audience_seen_csr
    ptr, flat = audience_seen_csr(seen, table.shape[0] - 1)
    q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(torch.int32)
    rows, sc = torch.zeros(q.numel(), k, dtype=torch.int32), torch.zeros(q.numel(), k)
    e = None if elig is None else torch.from_numpy(np.concatenate([[0], np.asarray(elig)]).astype(np.uint8))
    AR.sim_topk_users(emb, q, table, torch.from_numpy(ptr), torch.from_numpy(flat), e, k, rows, sc)
    return rows.numpy().astype(np.int64) - 1, sc.numpy()


def test_user_vectors_are_the_vectors_recommend_scores_with(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users
    from topk_ref import sim_topk_items
    from adapter4rec_amd.data_utils.metrics import recommend, user_vectors
    model, args, item_num, emb, eval_seq, _ = _id_model_and_users(13)
    seen = []

    def keeping(prec, *a):
        seen.append(prec.clone())
        return sim_topk_items(prec, *a)
    monkeypatch.setattr(sim_lib, 'topk_items', keeping, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_users', _refuse)
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '5')
    recommend(model, eval_seq, emb, 4, args)
    uv = user_vectors(model, eval_seq, emb, args)
    assert uv.dtype == torch.float32 and tuple(uv.shape) == (13, emb.shape[1]) and [p.shape[0] for p in seen] == [5, 5, 3]
    assert torch.equal(uv, torch.cat(seen))                                        # the same inputs through the same code: the same bits
    assert torch.equal(user_vectors(model, eval_seq, emb, args, user_ids=[7, 2, 7]), uv[[7, 2, 7]])
    assert tuple(user_vectors(model, eval_seq, emb, args, user_ids=[]).shape) == (0, emb.shape[1])
    with pytest.raises(ValueError, match='empty sequence'):
        user_vectors(model, {**eval_seq, 3: []}, emb, args)


def test_audience_in_batches_against_the_restatement(simulated, monkeypatch):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import audience, audience_seen_csr, user_vectors
    model, args, item_num, emb, eval_seq, _ = _id_model_and_users(30)
    n, k = len(eval_seq), 6
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '32')
    ids, sc = audience(model, eval_seq, emb, k, args)
    want_q = [32] * (item_num // 32) + ([item_num % 32] if item_num % 32 else [])
    assert [c['Q'] for c in CALLS] == want_q and all(c['elig'] is None and c['k'] == k for c in CALLS)
    assert all(c['table'] is CALLS[0]['table'] and c['ptr'] is CALLS[0]['ptr'] for c in CALLS)      # the user table and the CSR: built once per call
    table, ptr, flat = CALLS[0]['table'], CALLS[0]['ptr'], CALLS[0]['flat']
    assert tuple(table.shape) == (n + 1, emb.shape[1]) and (table[0] == 0).all() and ptr.dtype == torch.int64 and flat.dtype == torch.int32
    assert torch.equal(table[1:], user_vectors(model, eval_seq, emb, args))
    p2, f2 = audience_seen_csr(eval_seq, n)
    assert ptr.tolist() == p2.tolist() and flat.tolist() == f2.tolist()             # seen defaults to the users' sequences
    assert ids.dtype == torch.long and sc.dtype == torch.float32 and tuple(ids.shape) == (item_num, k) == tuple(sc.shape)
    query = np.arange(1, item_num + 1)
    ri, rs = AR.audience_reference(emb, table, query, k + 1, p2, f2)
    sure = AR.decided(rs, AR.bounds(emb, table, query).max(1))
    assert sure.mean() > 0.9
    np.testing.assert_array_equal(ids.numpy()[sure], ri[:, :k][sure] - 1)
    np.testing.assert_allclose(sc.numpy(), rs[:, :k], rtol=0, atol=1e-4)
    for u in range(n):                                                             # a user is never listed for an item of the user's sequence
        assert not (ids[np.asarray(eval_seq[u]) - 1] == u).any()
    si, ss = _sim_lists(emb, table, query, k, eval_seq)
    np.testing.assert_array_equal(ids.numpy(), si)
    # a query list (order, repeats, ids that are no item), seen lists of the caller's, eligible users: -1 pads
    CALLS.clear()
    seen = {u: [1, 2, 3] if u % 2 else list(range(1, item_num + 1)) for u in range(n)}      # even users have seen everything
    elig = np.zeros(n, bool)
    elig[[1, 4, 5, 9, 11]] = True
    query = torch.tensor([9, 2, 2, 0, item_num + 1, 17, -3])
    ids, sc = audience(model, eval_seq, emb, k, args, item_ids=query, seen=seen, eligible=torch.from_numpy(elig))
    assert [c['Q'] for c in CALLS] == [7] and CALLS[0]['elig'].dtype == torch.uint8 and CALLS[0]['elig'].tolist() == [0] + elig.astype(int).tolist()
    si, ss = _sim_lists(emb, table, query.numpy(), k, seen, elig)
    np.testing.assert_array_equal(ids.numpy(), si)
    np.testing.assert_array_equal(sc.numpy(), ss)
    assert set(ids[0].tolist()) == {1, 5, 9, 11, -1} and (ids[0, 4:] == -1).all() and torch.isneginf(sc[0, 4:]).all()
    assert (ids[1] == -1).all() and torch.equal(ids[1], ids[2])                    # item 2: every eligible odd user has seen it
    assert (ids[[3, 4, 6]] == -1).all() and torch.isneginf(sc[[3, 4, 6]]).all()
    assert tuple(audience(model, eval_seq, emb, k, args, item_ids=[])[0].shape) == (0, k)
    with pytest.raises(ValueError, match='one entry per user'):
        audience(model, eval_seq, emb, k, args, eligible=np.ones(n + 1, bool))


def test_write_audience_file_and_log(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from adapter4rec_amd.data_utils.metrics import user_vectors, write_audience
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(30)
    n, k = len(eval_seq), 4
    hist[3] = torch.LongTensor(np.arange(1, item_num + 1))                         # a history far beyond recommend's 264-id cap would be: here, everything
    user_names = [f'U{u:02d}' for u in range(n)]
    item_names = [None] + [f'I{i:03d}' for i in range(1, item_num + 1)]
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '16')
    path, log = str(tmp_path / 'all.tsv'), _Log()
    assert write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path, Log_file=log) == path
    table = torch.cat([torch.zeros(1, emb.shape[1]), user_vectors(model, eval_seq, emb, args)])
    seen = [np.concatenate([np.asarray(hist[u]), np.asarray(eval_seq[u][-1:])]) for u in range(n)]
    si, ss = _sim_lists(emb, table, np.arange(1, item_num + 1), k, seen)
    rows = [l.rstrip('\n').split('\t') for l in open(path)]
    assert [r[0] for r in rows] == item_names[1:] and all(len(r) == 3 for r in rows)
    for i, r in enumerate(rows):
        assert r[1].split(' ') == [user_names[u] for u in si[i]] and 'U03' not in r[1].split(' ')
        assert r[2].split(' ') == ['%.9g' % float(s) for s in ss[i]]
        assert [np.float32(x) for x in r[2].split(' ')] == ss[i].tolist()          # %.9g round-trips fp32
    assert len(log.lines) == 1
    m = re.fullmatch(rf'audience   top-4 lists of {item_num} items over 30 users \(30 eligible\), {item_num} with a user, mean best score (-?\d+\.\d{{5}}) -> (.*)', log.lines[0])
    assert m and m.group(2) == path and abs(float(m.group(1)) - float(ss[:, 0].astype(np.float64).mean())) < 2e-5
    # query items in their order, two eligible users: short lists without pads, an item neither may see gets no line
    elig = np.zeros(n, bool)
    elig[[3, 8]] = True
    query = np.array([9, 2, int(eval_seq[8][-1]), 17])
    path2 = str(tmp_path / 'some.tsv')
    write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path2, item_ids=query, eligible=elig, Log_file=log)
    si, ss = _sim_lists(emb, table, query, k, seen, elig)
    keep = [r for r in range(4) if si[r, 0] >= 0]
    rows = [l.rstrip('\n').split('\t') for l in open(path2)]
    assert [r[0] for r in rows] == [item_names[int(query[r])] for r in keep] and 0 < len(keep) < 4 and 2 not in keep
    assert all(r[1] == 'U08' and len(r[2].split(' ')) == 1 for r in rows)
    assert log.lines[1].startswith(f'audience   top-4 lists of 4 items over 30 users (2 eligible), {len(keep)} with a user, mean best score ')
    with pytest.raises(ValueError, match='no query item'):
        write_audience(model, eval_seq, hist, emb, k, 16, args, user_names, item_names, path2, item_ids=np.zeros(0, np.int64))


def test_other_modes_never_call_the_new_entry(simulated, monkeypatch, tmp_path):
    from test_candidates_cpu import _id_model_and_users
    from similar_ref import sim_row_inv_norms, sim_topk_similar
    from topk_ref import sim_topk_items
    from adapter4rec_amd.data_utils.metrics import audience, eval_model, recommend, similar_items, write_recommendations
    monkeypatch.setattr(sim_lib, 'topk_users', _refuse)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_similar', sim_topk_similar, raising=False)
    monkeypatch.setattr(sim_lib, 'row_inv_norms', sim_row_inv_norms, raising=False)
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(12)
    seqs = {u: eval_seq[u][:-1] for u in eval_seq}
    recommend(model, seqs, emb, 5, args)
    similar_items(emb, 5)
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    write_recommendations(model, eval_seq, hist, emb, 5, 16, args, [f'U{u}' for u in seqs], names, str(tmp_path / 'r.tsv'), Log_file=_Log())
    eval_model(model, hist, eval_seq, emb, 16, args, item_num, logging.getLogger('t'), 'test', 0)
    with pytest.raises(AssertionError, match='audience entry called'):
        audience(model, eval_seq, emb, 5, args)


# ------------------------------------------------------------------ the entry point
def test_cv_id_runner_mode_audience(tmp_path, monkeypatch):
    """the image entry point with --item_tower id: train one epoch with the new entry refusing every call, then --mode audience from its checkpoint,
    to the default path; then query and user files to another path"""
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    from topk_ref import sim_topk_items
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.data_utils import read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    for name in ('id_index', 'id_grad_sum', 'id_index_ws_ints'):
        if hasattr(IC, name):
            monkeypatch.setattr(sim_lib, name, getattr(IC, name), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_users', _refuse, raising=False)
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    CALLS.clear()
    monkeypatch.setattr(sim_lib, 'topk_users', _recording)
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
    CR._run_cv(common + ['--mode', 'audience', '--load_ckpt_name', 'epoch-1.pt', '--topk', '3'], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == []                                # no training step, no evaluation
    out = os.path.join(os.path.dirname(ck[0]), 'audience_epoch-1.pt.tsv')
    keys, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    user_names, item_names = read_behavior_names(os.path.join(data, 'toy', 'users_log.tsv'), name2id, 20, 5)
    N, n = len(item_names) - 1, len(user_names)
    emb, table, ptr, flat = CALLS[0]['emb'], CALLS[0]['table'], CALLS[0]['ptr'], CALLS[0]['flat']
    assert tuple(table.shape) == (n + 1, emb.shape[1]) and emb.shape[0] == N + 1 and sum(c['Q'] for c in CALLS) >= N

    def check(path, query, k, elig):
        q = torch.as_tensor(np.asarray(query, dtype=np.int64)).to(torch.int32)
        rows, sc = torch.zeros(q.numel(), k, dtype=torch.int32), torch.zeros(q.numel(), k)
        AR.sim_topk_users(emb, q, table, ptr, flat, elig, k, rows, sc)
        want = []
        for r in range(q.numel()):
            keep = rows[r] != 0
            if keep.any():
                want.append([item_names[int(q[r])], ' '.join(user_names[int(u) - 1] for u in rows[r][keep]), ' '.join('%.9g' % float(s) for s in sc[r][keep])])
        got = [l.rstrip('\n').split('\t') for l in open(path)]
        assert got == want and len(got) > 0
        return got
    rows = check(out, np.arange(1, N + 1), 3, None)
    line = [l for l in seen_lines if l.startswith('audience   ')]
    assert len(line) == 1 and line[0].startswith(f'audience   top-3 lists of {N} items over {n} users ({n} eligible), {len(rows)} with a user, mean best score ')
    assert line[0].endswith('/audience_epoch-1.pt.tsv')
    lists = [flat[int(ptr[r]):int(ptr[r + 1])].tolist() for r in range(n + 1)]     # what the run took as seen: sorted, each id once, row 0 empty
    assert lists[0] == [] and all(l == sorted(set(l)) and len(l) >= 5 for l in lists[1:])
    by_item = {r[0]: r[1].split(' ') for r in rows}
    for u in range(n):
        for i in lists[u + 1]:
            assert user_names[u] not in by_item.get(item_names[i], [])
    # query items and eligible users from files, another path
    q_ids, u_ids = [7, 3, 11], [u for u in range(n) if u % 3]
    open(os.path.join(root, 'q.txt'), 'w').write('\n'.join(item_names[i] for i in q_ids + [7]) + '\n')
    open(os.path.join(root, 'u.txt'), 'w').write('\n'.join(user_names[u] for u in u_ids) + '\n')
    out2 = os.path.join(root, 'some.tsv')
    CALLS.clear()
    CR._run_cv(common + ['--mode', 'audience', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--audience_out', out2, '--audience_items', os.path.join(root, 'q.txt'),
                         '--audience_users', os.path.join(root, 'u.txt')], monkeypatch, rec)
    elig = torch.zeros(n + 1, dtype=torch.uint8)
    elig[[u + 1 for u in u_ids]] = 1
    assert torch.equal(CALLS[0]['elig'], elig) and torch.equal(CALLS[0]['table'], table)
    rows = check(out2, q_ids, 5, elig)
    assert all(set(r[1].split(' ')) <= {user_names[u] for u in u_ids} for r in rows)
    assert any(l.startswith(f'audience items: 3 of {N} from ') for l in seen_lines) and any(l.startswith(f'audience users: {len(u_ids)} of {n} from ') for l in seen_lines)
    open(os.path.join(root, 'u.txt'), 'w').write('ghost\n')
    with pytest.raises(ValueError, match='1 name.s. that are no user of this dataset: ghost'):
        CR._run_cv(common + ['--mode', 'audience', '--load_ckpt_name', 'epoch-1.pt', '--audience_users', os.path.join(root, 'u.txt')], monkeypatch, rec)
