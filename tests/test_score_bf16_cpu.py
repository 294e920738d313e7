"""CPU side of evaluation and top-K on the bf16 MFMA (include/a4r_score_bf16.h: a4r_eval_rank_bf16, a4r_topk_items_bf16, a4r_topk_bf16_ws_bytes): the
C boundary of the three exports (header, the binding's table in adapter4rec_amd/_lib_score_bf16.py, the built library, refusals before any
launch), the wrappers' refusals, --score_dtype in both parsers and its five refusals, the restatement (tests/score_bf16_ref.py) on a hand-made
case, the share of the random tables' positions the gap rule decides, and eval_model / recommend under score_dtype='bf16' on simulated kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import score_bf16_ref as SR
import sim_lib
from score_ce_bf16_ref import round_bf16
from topk_ref import sim_topk_items

NAMES = ['a4r_eval_rank_bf16', 'a4r_topk_bf16_ws_bytes', 'a4r_topk_items_bf16']


# ------------------------------------------------------------------ the C boundary, held as tests/test_abi_cpu.py holds include/a4r.h
def bf16_prototypes():
    import test_abi_cpu as ABI
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', ABI.header(('include', 'a4r_score_bf16.h'))):
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
    protos = bf16_prototypes()
    table = L.SCORE_BF16_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    assert not set(table) & set(L.SIGNATURES)
    for module, (other, _) in L.SATELLITES.items():
        if other != 'SCORE_BF16_SIGNATURES':
            assert not set(table) & set(getattr(L, other)), module
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    # the candidate entries' argument lists (the mask in front of the outputs), the operands untyped
    for bf, masked in (('a4r_eval_rank_bf16', 'a4r_eval_rank_cand'), ('a4r_topk_items_bf16', 'a4r_topk_items_cand')):
        assert table[bf] == L.CANDIDATES_SIGNATURES[masked], bf
        assert [p for p, _ in protos[bf][1]][1:3] == ['void', 'void']
    assert table['a4r_topk_bf16_ws_bytes'] == (ctypes.c_size_t, (ctypes.c_int,) * 4)
    txt = ABI.header(('include', 'a4r_score_bf16.h'))
    assert 'typedef' not in txt and '#define A4R_' not in txt.replace('#define A4R_SCORE_BF16_H', '')
    assert 'cast' not in ''.join(protos)                                           # the cast stays a4r_score_ce_bf16_cast
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert '#include "a4r_score_bf16.h"' in a4r_h                                  # one public header reaches all
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_eval_rank_bf16(*([None] * 8), 16.0, 100, 64)
    mk = open(os.path.join(ABI.ROOT, 'adapter4rec_amd', 'csrc', 'Makefile')).read()
    assert all('a4r_score_bf16.h' in l for l in mk.splitlines() if l.startswith(('%.o:', '%.w4.o:', '$(OPS_LIB):')))


def test_wrappers_are_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_score_bf16 as B
    assert L.eval_rank_bf16 is B.eval_rank_bf16 and L.topk_items_bf16 is B.topk_items_bf16 and L.topk_bf16_ws_bytes is B.topk_bf16_ws_bytes
    assert L.SCORE_BF16_SIGNATURES is B.SCORE_BF16_SIGNATURES
    with pytest.raises(AttributeError):
        L.eval_rank_bfloat16


def _exports():
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    out = {}
    for name, (restype, argtypes) in L.SCORE_BF16_SIGNATURES.items():
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
        out[name] = f
    return out


def test_exports_refuse_bad_arguments_before_launching():
    """With valid shapes and host addresses for the other pointers: each required pointer in turn NULL (the stream aside: NULL is the default
    stream; cand aside: NULL means all items), all NULL, every scalar out of its set, operands off 16 bytes, ws off 8 bytes -- A4R_EINVAL in front
    of the first HIP call, so nothing is enqueued and no GPU is needed.  The workspace query returns 0 for the same shapes."""
    f = _exports()
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    rank, topk, ws = f['a4r_eval_rank_bf16'], f['a4r_topk_items_bf16'], f['a4r_topk_bf16_ws_bytes']
    CAND = {'a4r_eval_rank_bf16': 6, 'a4r_topk_items_bf16': 5}
    probed = 0
    for name, fn, scalars in (('a4r_eval_rank_bf16', rank, (16, 100, 64)), ('a4r_topk_items_bf16', topk, (16, 100, 64, 10))):
        n_ptr = len(fn.argtypes) - len(scalars)
        assert fn(*([None] * n_ptr), *scalars) == -1 and fn(*([None] * n_ptr), *([0] * len(scalars))) == -1, name
        for i in range(1, n_ptr):
            if i == CAND[name]:
                continue
            for cand in (None, p16):
                ptrs = [None] + [p16] * (n_ptr - 1)
                ptrs[CAND[name]] = cand
                ptrs[i] = None
                assert fn(*ptrs, *scalars) == -1, (name, i)
                probed += 1
    assert probed == 2 * (6 + 7)
    ok_r = [None] + [p16] * 7
    ok_t = [None] + [p16] * 8
    for U, N1, E in ((0, 100, 64), (-1, 100, 64), (16, 1, 64), (16, 0, 64), (16, 100, 0), (16, 100, 32), (16, 100, 96), (16, 100, 1024)):
        assert rank(*ok_r, U, N1, E) == -1, (U, N1, E)
        assert topk(*ok_t, U, N1, E, 10) == -1, (U, N1, E)
        assert ws(U, N1, E, 10) == 0, (U, N1, E)
    for K in (0, -1, 257):
        assert topk(*ok_t, 16, 100, 64, K) == -1 and ws(16, 100, 64, K) == 0, K
    for at in (1, 2):                                                              # prec_b / table_b off 16 bytes
        for off in (2, 8):
            bad = list(ok_r)
            bad[at] = p16 + off
            assert rank(*bad, 16, 100, 64) == -1
            bad = list(ok_t)
            bad[at] = p16 + off
            assert topk(*bad, 16, 100, 64, 10) == -1
    bad = list(ok_t)
    bad[8] = p16 + 4                                                               # ws off 8 bytes
    assert topk(*bad, 16, 100, 64, 10) == -1


def test_workspace_follows_the_grid():
    """gy x U x K keys of 8 bytes with 1 <= gy <= 32 item ranges, never more ranges than 4-tile groups of the table; every served shape > 0."""
    ws = _exports()['a4r_topk_bf16_ws_bytes']
    for U in (1, 16, 17, 64, 65, 4096, 32768):
        for N1 in (2, 17, 66, 14720, 65537, 500001):
            for E in (64, 128, 256, 512):
                for K in (1, 10, 64, 65, 100, 256):
                    b = ws(U, N1, E, K)
                    assert b > 0 and b % (8 * U * K) == 0, (U, N1, E, K)
                    gy = b // (8 * U * K)
                    assert 1 <= gy <= 32 and gy <= ((N1 - 1 + 15) // 16 + 3) // 4, (U, N1, E, K, gy)
    assert ws(1, 500001, 64, 10) == 32 * 8 * 10 and ws(32768, 65537, 64, 256) == 8 * 32768 * 256


# ------------------------------------------------------------------ the wrappers' refusals
def test_wrappers_refuse_bad_arguments(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the checks on host tensors
    N1, U, E, k = 9, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)

    def rank(**kw):
        a = dict(prec_b=bf(U, E), table_b=bf(N1, E), target=i32(U), hist_ptr=i32(U + 1), hist_idx=i32(1), rank=i32(U), cand=None)
        a.update(kw)
        return L.eval_rank_bf16(**a)

    def topk(**kw):
        a = dict(prec_b=bf(U, E), table_b=bf(N1, E), excl_ptr=i32(U + 1), excl_idx=i32(1), k=k, ids=i32(U, k), scores=torch.zeros(U, k), cand=None)
        a.update(kw)
        return L.topk_items_bf16(**a)

    operands = [(dict(prec_b=torch.zeros(U, E)), 'bf16'), (dict(table_b=torch.zeros(N1, E)), 'bf16'), (dict(prec_b=bf(U, E).half()), 'bf16'),
                (dict(prec_b=bf(U, 2 * E)[:, ::2]), 'contiguous'), (dict(table_b=bf(N1, 128)), 'expected'), (dict(prec_b=bf(U)), 'expected'),
                (dict(prec_b=bf(U, 96), table_b=bf(N1, 96)), 'E = 96'), (dict(table_b=bf(1, E)), 'N1 >= 2'), (dict(prec_b=bf(0, E)), 'U >= 1'),
                (dict(prec_b=bf(U + 1, E).view(-1)[4:4 + U * E].view(U, E)), '16-byte'),
                (dict(cand=torch.ones(N1, dtype=torch.int32)), 'uint8 or bool'), (dict(cand=torch.ones(N1 - 1, dtype=torch.uint8)), 'one entry per table row'),
                (dict(cand=np.ones(N1, np.uint8)), 'tensor'), (dict(cand=torch.ones(N1, dtype=torch.bool)), 'device tensor')]
    for f in (rank, topk):
        for bad, msg in operands:
            with pytest.raises(ValueError, match=msg):
                f(**bad)
    for bad, msg in ((dict(target=torch.zeros(U, dtype=torch.int64)), 'target'), (dict(hist_ptr=i32(U)), 'hist_ptr'), (dict(rank=i32(U - 1)), 'rank'),
                     (dict(hist_idx=i32(0)), 'hist_idx'), (dict(rank=torch.zeros(U)), 'rank')):
        with pytest.raises(ValueError, match=msg):
            rank(**bad)
    for bad, msg in ((dict(k=0), 'outside'), (dict(k=257), 'outside'), (dict(excl_ptr=i32(U)), 'U \\+ 1'), (dict(ids=i32(U, 2)), 'must be'),
                     (dict(excl_idx=torch.zeros(1, dtype=torch.int64)), 'int32'), (dict(scores=torch.zeros(U, k, dtype=torch.float64)), 'fp32')):
        with pytest.raises(ValueError, match=msg):
            topk(**bad)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match='device tensors'):                       # no CPU fallback
        rank()
    with pytest.raises(RuntimeError, match='device tensors'):
        topk()


# ------------------------------------------------------------------ flags
def test_both_parsers_take_the_flag():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        assert parse([]).score_dtype == 'fp32' and parse(['--mode', 'test']).score_dtype == 'fp32'
        assert parse(['--mode', 'recommend', '--score_dtype', 'bf16']).score_dtype == 'bf16'
        assert parse(['--score_dtype', 'bf16']).mode == 'train'
        with pytest.raises(SystemExit):
            parse(['--score_dtype', 'fp16'])


REFUSALS = [(['--mode', 'test', '--candidate_lists', 'l.tsv'], '--candidate_lists'), (['--mode', 'recommend', '--candidate_lists', 'l.tsv'], '--candidate_lists'),
            (['--mode', 'test', '--eval_negatives', '100'], '--eval_negatives'), (['--mode', 'train', '--eval_negatives', '100'], '--eval_negatives'),
            (['--mode', 'recommend', '--diversify', 'mmr'], '--diversify'), (['--mode', 'similar'], '--mode similar'),
            (['--mode', 'similar', '--candidate_items', 'c.txt'], '--mode similar')]


@pytest.mark.parametrize('flags,what', REFUSALS)
def test_flag_is_refused_beside_the_fp32_only_paths(flags, what):
    """Before anything is set up (no device, no process group), in both entry points; without --score_dtype bf16 the same flags pass the check."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.data_utils.eval_flags import check_flags
    from adapter4rec_amd.parameters import parse_args
    for main in (run.main, run_adapter.main):
        with pytest.raises(ValueError, match='--score_dtype bf16.*' + re.escape(what)):
            main(flags + ['--score_dtype', 'bf16'])
    for parse in (parse_args, cv_parse):
        check_flags(parse(flags))
        check_flags(parse(flags + ['--score_dtype', 'fp32']))


def test_flag_is_honoured_by_the_other_modes():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.data_utils.eval_flags import check_flags, score_dtype_from_args
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        for flags in (['--mode', 'test'], ['--mode', 'train'], ['--mode', 'recommend'], ['--mode', 'test', '--candidate_items', 'c.txt'],
                      ['--mode', 'recommend', '--candidate_items', 'c.txt'], ['--mode', 'train', '--loss', 'ce', '--ce_dtype', 'bf16'],
                      ['--mode', 'train', '--loss', 'ce', '--ce_dtype', 'fp32']):
            try:
                args = parse(flags + ['--score_dtype', 'bf16'])
            except SystemExit:                                                     # (a parser without --loss / --ce_dtype)
                continue
            check_flags(args)
            log = _Log()
            assert score_dtype_from_args(args, log) == dict(score_dtype='bf16')
            assert len(log.lines) == 1 and 'bf16' in log.lines[0]                  # the log line names the dtype
            log = _Log()
            assert score_dtype_from_args(parse(flags), log) == {} and log.lines == []


def test_metrics_refuse_the_fp32_only_restrictions():
    from adapter4rec_amd.data_utils import metrics as M
    with pytest.raises(ValueError, match='expected one of'):
        M._score_dtype_checked('fp16')
    assert M._score_dtype_checked('fp32', candidate_lists={0: [1]}, eval_negatives=object(), diversify=object()) == 'fp32'
    assert M._score_dtype_checked('bf16', candidate_lists=None, eval_negatives=None, diversify=None) == 'bf16'
    for name in ('candidate_lists', 'eval_negatives', 'diversify'):
        with pytest.raises(ValueError, match=f'bf16.*{name}'):
            M._score_dtype_checked('bf16', **{name: object()})


# ------------------------------------------------------------------ the restatement
def test_restatement_on_a_hand_made_case():
    """Two items whose fp32 rows differ below bf16's resolution tie after rounding (the smaller id first), an item that wins in fp32 loses after
    rounding, and the rank counts strictly greater scores at the rounded operands."""
    e = np.zeros((6, 64), np.float32)
    e[1, 0], e[2, 0], e[3, 0], e[4, 0], e[5, 0] = 1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -7, 0.5, 1.0 + 2.0 ** -9
    p = np.zeros((1, 64), np.float32)
    p[0, 0] = 1.0 + 2.0 ** -12                                                       # rounds to 1
    assert round_bf16(e[:, 0]).tolist() == [0.0, 1.0, 1.0, 1.0 + 2.0 ** -7, 0.5, 1.0]  # (bf16 keeps 7 fraction bits)
    s = SR.scores64(p, e)
    assert s[0].tolist() == [0.0, 1.0, 1.0, 1.0078125, 0.5, 1.0]
    i, v = SR.topk_reference_cand(s, [[]], 5)
    assert i.tolist() == [[3, 1, 2, 5, 4]] and v[0].tolist() == [1.0078125, 1.0, 1.0, 1.0, 0.5]
    s32 = p.astype(np.float64) @ e.astype(np.float64).T                              # the fp32 entries' order differs: 3, 5, 2, 1, 4
    assert SR.topk_reference_cand(s32, [[]], 5)[0].tolist() == [[3, 5, 2, 1, 4]]
    assert SR.rank_reference(s, [1], [[]]).tolist() == [2] and SR.rank_reference(s32, [1], [[]]).tolist() == [4]
    assert SR.rank_reference(s, [4], [[3, 3, 0, 99]]).tolist() == [4]
    cand = np.array([1, 0, 1, 0, 1, 1])
    assert SR.rank_reference(s, [1], [[]], cand).tolist() == [1]                     # 3 is no candidate; the target need not be one
    assert SR.topk_reference_cand(s, [[5]], 4, cand)[0].tolist() == [[2, 4, 0, 0]]
    lo, hi = SR.rank_interval(s, np.full_like(s, 1e-3), [1], [[]])
    assert (lo.tolist(), hi.tolist()) == ([2], [5])                                  # 3 is above by more than 2b; 2 and 5 (equal) and 1 itself within
    assert SR.hit_ndcg([1, 3, 11]) == (2 / 3, (1.0 + 0.5) / 3)
    # the bound: E x 2^-24 x sum |a b| at the rounded operands
    assert SR.sum_bound(p, e)[0, 3] == 64 * 2.0 ** -24 * 1.0078125


@pytest.mark.parametrize('K,E,floor', [(10, 64, 0.95), (100, 128, 0.9), (256, 512, 0.5)])
def test_random_cases_are_decided_by_the_gap_rule(K, E, floor):
    """The random tables of tests/test_score_bf16_gpu.py, from the fp64 reference alone: the share of list positions separated from both
    neighbours by more than the summation bound (1.00 / 0.97 / 0.67 at the three shapes) -- at least half everywhere, what the GPU test asks."""
    c = SR.random_case(K, E)
    share = float(c['sure'].mean())
    print(f'K = {K}, E = {E}: {share:.3f} of the positions decided')
    assert c['sure'].shape == (64, K) and share >= floor >= 0.5, share
    lo, hi = SR.rank_interval(c['s64'], c['bound'], c['target'], c['lists'])
    print(f'rank intervals: widest {int((hi - lo).max())} of {SR.RANDOM_N1 - 1} items')
    assert (lo <= hi).all() and (hi - lo).max() < 0.002 * SR.RANDOM_N1            # the rank check has teeth: an interval is a few ranks wide


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def _recording(name, fn):
    def call(*a, **k):
        CALLS.append((name, [x.detach().clone() if isinstance(x, torch.Tensor) else x for x in a], dict(k)))
        return fn(*a, **k)
    return call


def _refuse(*a, **k):
    raise AssertionError('an fp32 entry under score_dtype bf16 / a bf16 entry under the default')


FP32_ENTRIES = ('eval_rank', 'eval_rank_cand', 'topk_items', 'topk_items_cand')
BF16_ENTRIES = ('eval_rank_bf16', 'topk_items_bf16', 'cast_bf16')


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    import test_candidates_cpu as TC
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', TC.sim_eval_rank_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', TC.sim_topk_items_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_bf16', _recording('rank', SR.sim_eval_rank_bf16), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_bf16', _recording('topk', SR.sim_topk_items_bf16), raising=False)
    monkeypatch.setattr(sim_lib, 'cast_bf16', _recording('cast', SR.sim_cast_bf16), raising=False)
    CALLS.clear()


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def _model():
    import test_candidates_cpu as TC
    return TC._id_model_and_users(41)


def _precs(kind):
    """the fp32 user vectors handed to the cast (every cast but the table's), and the bf16 ones handed to the entry"""
    casts = [c[1][0] for c in CALLS if c[0] == 'cast']
    entry = [c[1][0] for c in CALLS if c[0] == kind]
    return casts, entry


@pytest.mark.parametrize('masked', [False, True])
def test_eval_model_bf16_against_the_restatement(simulated, monkeypatch, masked):
    from adapter4rec_amd.data_utils.metrics import eval_model, eval_ranks
    model, args, item_num, emb, eval_seq, hist = _model()
    U = len(eval_seq)
    target = np.array([eval_seq[u][-1] for u in range(U)])
    hlists = [hist[u].numpy() for u in range(U)]
    cand = None
    if masked:
        cand = np.random.default_rng(5).random(item_num + 1) < 0.6
        cand[target] = True                                                          # every user counts: the means run over all of them
    for name in FP32_ENTRIES:
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)                   # under bf16, no fp32 entry is ever called
    ranks = eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidates=cand, score_dtype='bf16').numpy()
    casts, entry = _precs('rank')
    assert len(casts) == 1 + len(entry) and casts[0].shape == emb.shape and torch.equal(casts[0], emb)      # the table once, each batch's prec once
    prec = torch.cat(casts[1:]).numpy()
    assert prec.shape == (U, emb.shape[1]) and prec.dtype == np.float32
    for c in CALLS:
        if c[0] == 'rank':
            assert c[1][0].dtype == torch.bfloat16 and c[1][1].dtype == torch.bfloat16 and c[1][1].shape == emb.shape
            assert (c[1][6] is None) == (not masked)
    got_b = torch.cat(entry).float().numpy()
    np.testing.assert_array_equal(got_b.view(np.uint32), round_bf16(prec).view(np.uint32))                   # the entry saw the rounded vectors
    s64 = SR.scores64(prec, emb.numpy())
    want = SR.rank_reference(s64, target, hlists, cand)
    np.testing.assert_array_equal(ranks, want)
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', candidates=cand, score_dtype='bf16')
    hit, ndcg = SR.hit_ndcg(want)
    assert abs(hr - hit) < 1e-6
    line = [l for l in log.lines if 'test_results' in l][0]
    np.testing.assert_allclose([float(x) for x in line.split()[1:]], [hit * 100, ndcg * 100], atol=1e-4)
    for kw in (dict(candidate_lists={0: [1, 2]}), dict(eval_negatives=object())):
        with pytest.raises(ValueError, match='bf16'):
            eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', score_dtype='bf16', **kw)
    with pytest.raises(ValueError, match='expected one of'):
        eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', score_dtype='half')


@pytest.mark.parametrize('masked', [False, True])
def test_recommend_bf16_against_the_restatement(simulated, monkeypatch, masked, tmp_path):
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend, write_recommendations
    model, args, item_num, emb, eval_seq, hist = _model()
    U, k = len(eval_seq), 10
    cand = (np.random.default_rng(6).random(item_num + 1) < 0.5) if masked else None
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    for name in FP32_ENTRIES:
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)
    ids, sc = recommend(model, seqs, emb, k, args, candidates=cand, score_dtype='bf16')
    casts, entry = _precs('topk')
    assert len(casts) == 1 + len(entry) == 2 and torch.equal(casts[0], emb)
    prec = torch.cat(casts[1:]).numpy()
    call = [c for c in CALLS if c[0] == 'topk'][0]
    assert call[1][0].dtype == torch.bfloat16 and call[1][1].dtype == torch.bfloat16 and (call[1][7] is None) == (not masked)
    s64 = SR.scores64(prec, emb.numpy())
    ri, rs = SR.topk_reference_cand(s64, [seqs[u] for u in range(U)], k, cand)
    np.testing.assert_array_equal(ids.numpy(), ri)
    np.testing.assert_array_equal(sc.numpy(), rs.astype(np.float32))
    # the scores are those of the rounded operands, not the fp32 ones
    s32 = prec.astype(np.float64) @ emb.double().numpy().T
    assert np.abs(np.take_along_axis(s32, ri, 1) - rs)[ri != 0].max() > 1e-4 * np.abs(rs[ri != 0]).max()
    for kw in (dict(candidate_lists={0: [1, 2]}), dict(diversify=Diversify(0.5, 20))):
        with pytest.raises(ValueError, match='bf16'):
            recommend(model, seqs, emb, k, args, score_dtype='bf16', **kw)
    # the runners' writer passes the dtype through: its file holds the restatement's lists (the held-out item excluded beside the history)
    names = [None] + [f'N{i}' for i in range(1, item_num + 1)]
    out = write_recommendations(model, eval_seq, hist, emb, 5, 16, args, [f'U{u}' for u in range(U)], names, str(tmp_path / 'r.tsv'),
                                candidates=cand, score_dtype='bf16')
    precs = {}
    for c in [c for c in CALLS if c[0] == 'cast'][2:]:
        if c[1][0].shape != emb.shape:
            precs[len(precs)] = c[1][0]
    lines = [l.rstrip('\n').split('\t') for l in open(out)]
    assert [l[0] for l in lines] == [f'U{u}' for u in range(U)]
    s64w = SR.scores64(torch.cat(list(precs.values())).numpy()[:U], emb.numpy())
    wi, _ = SR.topk_reference_cand(s64w, [eval_seq[u] for u in range(U)], 5, cand)
    for u, l in enumerate(lines):
        assert (l[1].split(' ') if l[1] else []) == [names[i] for i in wi[u] if i != 0], u


def test_under_the_default_no_new_entry_is_called(simulated, monkeypatch):
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend
    model, args, item_num, emb, eval_seq, hist = _model()
    for name in BF16_ENTRIES:
        monkeypatch.setattr(sim_lib, name, _refuse, raising=False)
    seqs = {u: eval_seq[u][:-1] for u in eval_seq}
    ones = np.ones(item_num + 1, bool)
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu')
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', score_dtype='fp32') == hr
    assert abs(eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=ones) - hr) < 1e-7      # (sum / k, not .mean())
    a = recommend(model, seqs, emb, 5, args)
    b = recommend(model, seqs, emb, 5, args, score_dtype='fp32')
    c = recommend(model, seqs, emb, 5, args, candidates=ones)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0])
    assert CALLS == []
