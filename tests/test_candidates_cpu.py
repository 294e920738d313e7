"""CPU side of candidate sets (include/a4r_candidates.h: a4r_eval_rank_cand, a4r_topk_items_cand): the C boundary of the two exports (header, the
binding's table in adapter4rec_amd/_lib_candidates.py, the built library, NULL refusals), the wrappers' and the Python API's mask checks,
read_candidates, --candidate_items in both parsers and its refusal under --mode train, eval_model / recommend with a mask on simulated kernels
against the numpy restatement (tests/cand_ref.py), and the text runner's --mode recommend --candidate_items file."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import cand_ref as CR
import sim_lib
from topk_ref import sim_topk_items

NAMES = ['a4r_eval_rank_cand', 'a4r_topk_items_cand']


# ------------------------------------------------------------------ the C boundary, held as tests/test_abi_cpu.py holds include/a4r.h
def cand_prototypes():
    import test_abi_cpu as ABI
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', ABI.header(('include', 'a4r_candidates.h'))):
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
    protos = cand_prototypes()
    table = L.CANDIDATES_SIGNATURES
    assert sorted(table) == sorted(protos) == NAMES
    assert not set(table) & set(L.SIGNATURES) and not set(table) & set(L.SCORE_CE_BF16_SIGNATURES)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    # the unmasked entries' argument lists with the mask in front of the outputs
    for masked, plain, at in (('a4r_eval_rank_cand', 'a4r_eval_rank', 6), ('a4r_topk_items_cand', 'a4r_topk_items', 5)):
        res, args = L.SIGNATURES[plain]
        assert table[masked] == (res, args[:at] + (ctypes.c_void_p,) + args[at:]), masked
        assert [p for p, _ in protos[masked][1]][at] == 'uint8_t' and protos[masked][1][at][1]
    txt = ABI.header(('include', 'a4r_candidates.h'))
    assert 'typedef' not in txt and '#define A4R_' not in txt.replace('#define A4R_CANDIDATES_H', '')
    a4r_h = open(os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()
    assert '#include "a4r_candidates.h"' in a4r_h                                 # one public header reaches all
    assert int(re.search(r'#define A4R_ABI_VERSION (\d+)', a4r_h).group(1)) == L.ABI_VERSION == 411
    assert not set(NAMES) & set(ABI.prototypes())                                  # a4r.h's own prototype list is what it was
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                                               # lib() installs the table when it loads the library
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_eval_rank_cand(*([None] * 8), 16.0, 100, 64)


def test_wrappers_are_reachable_under_both_modules():
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_candidates as B
    assert L.eval_rank_cand is B.eval_rank_cand and L.topk_items_cand is B.topk_items_cand and L.CANDIDATES_SIGNATURES is B.CANDIDATES_SIGNATURES
    with pytest.raises(AttributeError):
        L.eval_rank_candidates


def test_exports_refuse_every_null_pointer_before_launching():
    """With valid shapes and host addresses for the other pointers, each pointer in turn NULL (the stream aside: NULL is the default stream), and
    all of them NULL: A4R_EINVAL in front of the first HIP call, so nothing is enqueued and no GPU is needed."""
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16
    probed = 0
    for name, scalars in (('a4r_eval_rank_cand', (16, 100, 64)), ('a4r_topk_items_cand', (16, 100, 64, 10))):
        restype, argtypes = L.CANDIDATES_SIGNATURES[name]
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
        n_ptr = sum(t is ctypes.c_void_p for t in argtypes)
        assert argtypes[:n_ptr] == (ctypes.c_void_p,) * n_ptr and n_ptr + len(scalars) == len(argtypes)
        assert f(*([None] * n_ptr), *scalars) == -1, name
        assert f(*([None] * n_ptr), *([0] * len(scalars))) == -1, name
        for i in range(1, n_ptr):
            ptrs = [None] + [p16] * (n_ptr - 1)
            ptrs[i] = None
            assert f(*ptrs, *scalars) == -1, (name, i)
            probed += 1
    assert probed == 7 + 8


# ------------------------------------------------------------------ mask checks
def test_wrappers_refuse_bad_masks(monkeypatch):
    from adapter4rec_amd import _lib as L
    monkeypatch.setattr(L, 'require_gpu', lambda *t: None)                        # reach the mask checks on host tensors
    N1, U, E, k = 9, 4, 64, 3
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    rank = lambda m: L.eval_rank_cand(torch.zeros(U, E), torch.zeros(N1, E), i32(U), i32(U + 1), i32(1), m, i32(U))
    topk = lambda m: L.topk_items_cand(torch.zeros(U, E), torch.zeros(N1, E), i32(U + 1), i32(1), m, k, i32(U, k), torch.zeros(U, k))
    bad = [(None, 'tensor'), (np.ones(N1, np.uint8), 'tensor'), (torch.ones(N1, dtype=torch.int32), 'uint8 or bool'),
           (torch.ones(N1), 'uint8 or bool'), (torch.ones(N1 - 1, dtype=torch.uint8), 'one entry per table row'),
           (torch.ones(N1 + 1, dtype=torch.bool), 'one entry per table row'), (torch.ones(N1, 1, dtype=torch.uint8), 'one entry per table row'),
           (torch.ones(2 * N1, dtype=torch.uint8)[::2], 'contiguous'),
           (torch.ones(N1, dtype=torch.uint8), 'device tensor'), (torch.ones(N1, dtype=torch.bool), 'device tensor')]       # (a host mask)
    for f in (rank, topk):
        for m, msg in bad:
            with pytest.raises(ValueError, match=msg):
                f(m)
    with pytest.raises(ValueError, match='expected'):                              # topk_items' own checks still stand
        L.topk_items_cand(torch.zeros(U, E), torch.zeros(N1, 128), i32(U + 1), i32(1), torch.ones(N1, dtype=torch.uint8), k, i32(U, k),
                          torch.zeros(U, k))


def test_api_mask_checks():
    from adapter4rec_amd.data_utils.metrics import candidate_mask
    assert candidate_mask(None, 7, 'cpu') is None
    for m in (np.array([0, 1, 0, 0, 2, 0, 0]), np.array([True, False, False, False, False, False, True]), [0, 0, 0, 1, 0, 0, 0],
              torch.tensor([1, 0, 0, 0, 0, 0, 1], dtype=torch.uint8), torch.tensor([False, True, False, False, False, False, False])):
        got = candidate_mask(m, 7, 'cpu')
        assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (7,)
        assert (got != 0).tolist() == (np.asarray(m) != 0).tolist()
    b = torch.tensor([False, True, False, False, False, False, False])
    assert candidate_mask(b, 7, 'cpu').data_ptr() == b.data_ptr()                  # a bool tensor is a mask as it stands
    for m, msg in ((np.ones(6, bool), 'one entry per table row'), (np.ones(8, bool), 'one entry per table row'), (np.ones((7, 1), bool), 'one entry'),
                   (np.zeros(7, bool), 'no candidate'), (np.array([1, 0, 0, 0, 0, 0, 0]), 'no candidate'),
                   (torch.zeros(7, dtype=torch.uint8), 'no candidate'), (torch.ones(7), 'bool or uint8'), (torch.ones(7, dtype=torch.int64), 'bool or uint8')):
        with pytest.raises(ValueError, match=msg):
            candidate_mask(m, 7, 'cpu')


def test_read_candidates(tmp_path):
    from adapter4rec_amd.cv.data_utils import read_candidates as cv_read
    from adapter4rec_amd.data_utils.metrics import read_candidates
    assert cv_read is read_candidates
    names = [None, 'N7', 'N3', 'N12', 'N5']
    p = tmp_path / 'c.txt'
    p.write_text('N3\n\nN5\nN3\n  \nN12  \n')
    m = read_candidates(str(p), names)
    assert m.dtype == bool and m.tolist() == [False, False, True, True, True]
    p.write_text('N3\nN99\nX1\nN99\nX2\nX3\nX4\nX5\n')
    with pytest.raises(ValueError, match=r'6 name\(s\).*N99, X1, X2, X3, X4 \.\.\.'):
        read_candidates(str(p), names)
    p.write_text('None\n')                                                         # the pad item has no name
    with pytest.raises(ValueError, match='None'):
        read_candidates(str(p), names)
    p.write_text('\n')
    assert not read_candidates(str(p), names).any()


# ------------------------------------------------------------------ flags
def test_both_parsers_take_the_flag():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        assert parse([]).candidate_items is None and parse(['--mode', 'test']).candidate_items is None
        assert parse(['--mode', 'recommend', '--candidate_items', 'stock.txt']).candidate_items == 'stock.txt'


def test_flag_is_refused_under_mode_train():
    """Before anything is set up (no device, no process group): training and its per-epoch evaluation are not restricted by the flag."""
    from adapter4rec_amd import run
    from adapter4rec_amd.cv import run_adapter
    for main in (run.main, run_adapter.main):
        with pytest.raises(ValueError, match='--candidate_items'):
            main(['--mode', 'train', '--candidate_items', 'stock.txt'])
        with pytest.raises(ValueError, match='--candidate_items'):
            main(['--candidate_items', 'stock.txt'])
    with pytest.raises(ValueError, match='--candidate_items'):
        run.main(['--mode', 'load', '--candidate_items', 'stock.txt'])                # (the text runner's --mode load trains)


# ------------------------------------------------------------------ the Python API on simulated kernels
CALLS = []


def sim_eval_rank_cand(prec, item_emb, target, hist_ptr, hist_idx, cand, rank):
    """sim_lib.eval_rank with the non-candidates struck out beside the history."""
    assert cand.dtype == torch.uint8 and cand.is_contiguous() and cand.numel() == item_emb.shape[0]
    CALLS.append(('rank', prec.detach().clone(), target.clone()))
    sc = prec @ item_emb.t()
    for u in range(prec.shape[0]):
        s = sc[u].clone()
        ts = s[int(target[u])].item()
        s[hist_idx[int(hist_ptr[u]):int(hist_ptr[u + 1])].long()] = -float('inf')
        s[cand == 0] = -float('inf')
        rank[u] = int((s[1:] > ts).sum()) + 1


def sim_topk_items_cand(prec, item_emb, excl_ptr, excl_idx, cand, k, ids, scores):
    """The whole ordering of every user from the unmasked stand-in, the non-candidates dropped from it, cut to k."""
    assert cand.dtype == torch.uint8 and cand.is_contiguous() and cand.numel() == item_emb.shape[0]
    CALLS.append(('topk', prec.detach().clone(), None))
    U, N1 = prec.shape[0], item_emb.shape[0]
    full_i, full_s = torch.zeros(U, N1 - 1, dtype=torch.int32), torch.zeros(U, N1 - 1)
    sim_topk_items(prec, item_emb, excl_ptr, excl_idx, N1 - 1, full_i, full_s)
    ids.zero_()
    scores.fill_(-float('inf'))
    for u in range(U):
        keep = (full_i[u] != 0) & (cand[full_i[u].long()] != 0)
        n = min(int(k), int(keep.sum()))
        ids[u, :n] = full_i[u][keep][:n]
        scores[u, :n] = full_s[u][keep][:n]
    return ids, scores


def _refuse(*a, **k):
    raise AssertionError('an unmasked call under a candidate set / a masked call without one')


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.data_utils.metrics as M
    for mod in (E, EI, M):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', sim_eval_rank_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand, raising=False)
    CALLS.clear()


def _id_model_and_users(U=45):
    import test_id_tower_cpu as IC
    model, fx, _ = IC.build('sasrec', compute_dtype='fp32')
    args = IC.make_args(arch='sasrec', adapter_type='None')
    item_num = int(fx['item_num'])
    emb = model.state_dict()['id_embedding.weight'].detach().float().clone()
    rng = np.random.default_rng(11)
    eval_seq, hist = {}, {}
    for u in range(U):
        s = [int(x) for x in rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False)]
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    return model, args, item_num, emb, eval_seq, hist


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def test_eval_model_with_a_mask_against_the_restatement(simulated, monkeypatch):
    from adapter4rec_amd.data_utils.metrics import eval_model, eval_ranks
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(24)
    U = len(eval_seq)
    target = np.array([eval_seq[u][-1] for u in range(U)])
    rng = np.random.default_rng(12)
    cand = rng.random(item_num + 1) < 0.5
    cand[target[:5]] = False                                                      # users whose target is no candidate ...
    cand[target[5:10]] = True                                                     # ... and users whose target is one
    cand[target[:5]] = False
    hlists = [hist[u].numpy() for u in range(U)]
    assert any((~cand[h]).any() for h in hlists)                                  # history ids that are no candidates
    monkeypatch.setattr(sim_lib, 'eval_rank', _refuse)                            # under a mask, the unmasked entry is never called
    log = _Log()
    ranks = eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidates=cand).numpy()
    prec = torch.cat([c[1] for c in CALLS if c[0] == 'rank']).double().numpy()
    assert prec.shape[0] == U == len(ranks)                                       # ranks for every listed user, candidate target or not
    s64 = prec @ emb.double().numpy().T
    want = CR.rank_cand_reference(s64, target, hlists, cand)
    np.testing.assert_array_equal(ranks, want)
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', candidates=cand)
    hit, ndcg, n = CR.hit_ndcg_means(want, target, cand)
    assert 0 < n < U and abs(hr - hit) < 1e-7
    # the means run over the n users with a candidate target only: not over all users, whatever the others' ranks are
    all_users = float((want <= 10).mean())
    assert abs(hit - all_users) > 1e-3 or n == U
    line = [l for l in log.lines if 'test_results' in l][0]
    np.testing.assert_allclose([float(x) for x in line.split()[1:]], [hit * 100, ndcg * 100], atol=1e-4)
    assert any(f'{n} of {U} users' in l for l in log.lines)
    # the three mask forms give the same figure
    for m in (torch.from_numpy(cand), cand.astype(np.uint8), torch.from_numpy(cand.astype(np.uint8))):
        assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=m) == hr
    # no user qualifies / bad masks
    none = np.zeros(item_num + 1, bool)
    none[[i for i in range(1, item_num + 1) if i not in set(target.tolist())][:3]] = True
    with pytest.raises(ValueError, match='no user'):
        eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=none)
    with pytest.raises(ValueError, match='one entry per table row'):
        eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=cand[:-1])
    with pytest.raises(ValueError, match='no candidate'):
        eval_ranks(model, hist, eval_seq, emb, 16, args, list(range(U)), candidates=np.zeros(item_num + 1, bool))


def test_recommend_with_a_mask_against_the_restatement(simulated, monkeypatch):
    from adapter4rec_amd.data_utils.metrics import recommend
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(37)
    U, k = len(eval_seq), 10
    rng = np.random.default_rng(13)
    cand = rng.random(item_num + 1) < 0.4
    cand[0] = True                                                                # the pad entry is ignored
    seqs = {u: eval_seq[u][:-1] for u in range(U)}
    monkeypatch.setattr(sim_lib, 'topk_items', _refuse)
    ids, sc = recommend(model, seqs, emb, k, args, candidates=cand)
    prec = torch.cat([c[1] for c in CALLS if c[0] == 'topk']).double().numpy()
    s64 = prec @ emb.double().numpy().T
    ri, rs = CR.topk_cand_reference(s64, [seqs[u] for u in range(U)], cand, k)
    np.testing.assert_array_equal(ids.numpy(), ri)
    np.testing.assert_allclose(sc.numpy(), rs, rtol=0, atol=1e-5 * np.abs(s64).max())
    got = ids.numpy()
    assert cand[got[got != 0]].all() and (got != 0).any()
    for u in range(U):
        assert not set(got[u].tolist()) & set(seqs[u])
    # few candidates: short lists end in id 0 / -inf
    few = np.zeros(item_num + 1, bool)
    few[[3, 17, 41]] = True
    ids, sc = recommend(model, seqs, emb, k, args, candidates=few, user_ids=[0, 5, 6])
    ri, _ = CR.topk_cand_reference(s64[[0, 5, 6]], [seqs[u] for u in (0, 5, 6)], few, k)
    np.testing.assert_array_equal(ids.numpy(), ri)
    assert (ids[:, 3:] == 0).all() and torch.isinf(sc[:, 3:]).all()
    with pytest.raises(ValueError, match='one entry per table row'):
        recommend(model, seqs, emb, k, args, candidates=cand[1:])
    with pytest.raises(ValueError, match='no candidate'):
        recommend(model, seqs, emb, k, args, candidates=np.array([True] + [False] * item_num))


def test_without_candidates_the_masked_wrappers_are_never_called(simulated, monkeypatch):
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend
    model, args, item_num, emb, eval_seq, hist = _id_model_and_users(20)
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', _refuse)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', _refuse)
    log = _Log()
    hr = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu')
    hr_none = eval_model(model, hist, eval_seq, emb, 16, args, item_num, log, 'test', 'cpu', candidates=None)
    assert hr == hr_none and not any('users' in l for l in log.lines)
    a = recommend(model, {u: eval_seq[u][:-1] for u in eval_seq}, emb, 5, args)
    b = recommend(model, {u: eval_seq[u][:-1] for u in eval_seq}, emb, 5, args, candidates=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # an all-ones mask is the unmasked result (the stand-ins agree with each other)
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', sim_eval_rank_cand)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand)
    ones = np.ones(item_num + 1, bool)
    assert eval_model(model, hist, eval_seq, emb, 16, args, item_num, _Log(), 'test', 'cpu', candidates=ones) == hr
    c = recommend(model, {u: eval_seq[u][:-1] for u in eval_seq}, emb, 5, args, candidates=ones)
    assert torch.equal(a[0], c[0])


def test_restatement_semantics():
    """the restatement itself: the target need not be a candidate, a non-candidate history id changes nothing, cand[0] is ignored, lists keep
    topk_reference's order and padding"""
    s = np.array([[9.0, 1.0, 3.0, 3.0, 5.0, 2.0, 4.0]])
    cand = np.array([1, 0, 1, 1, 0, 1, 1])
    assert CR.rank_cand_reference(s, [1], [[]], cand).tolist() == [5]             # 2, 3, 5, 6 beat item 1, which is no candidate itself
    assert CR.rank_cand_reference(s, [5], [[4, 6]], cand).tolist() == [3]         # 2, 3; 4 is no candidate (nothing to take back), 6 is history
    assert CR.rank_cand_reference(s, [5], [[5, 0, 99, -1]], cand).tolist() == [4]
    i, v = CR.topk_cand_reference(s, [[6, 4, 0, 99]], cand, 5)
    assert i.tolist() == [[2, 3, 5, 0, 0]] and v[0, :3].tolist() == [3.0, 3.0, 2.0] and np.isinf(v[0, 3:]).all()
    cand0 = cand.copy()
    cand0[0] = 0
    assert np.array_equal(CR.topk_cand_reference(s, [[]], cand0, 4)[0], CR.topk_cand_reference(s, [[]], cand, 4)[0])
    assert CR.topk_cand_reference(s, [[]], np.zeros(7), 3)[0].tolist() == [[0, 0, 0]]
    assert CR.rank_cand_reference(s, [4], [[]], np.zeros(7)).tolist() == [1]
    # more than MAX_EXCL non-candidates: what a user's extended exclusion list could not say
    big = np.arange(1000, dtype=np.float64)[None]
    c = np.zeros(1000)
    c[[5, 700]] = 1
    assert CR.topk_cand_reference(big, [[700]], c, 2)[0].tolist() == [[5, 0]]


def test_random_case_is_decided_by_the_gap_rule():
    """The random-table case of tests/test_candidates_gpu.py, from the fp64 reference alone: at least 95 % of the list positions are separated
    from both neighbours by more than the fp32 summation bound, so the GPU test compares nearly every position."""
    prec, emb, cand, lists, target = CR.random_case()
    k = CR.RANDOM_CASE['K']
    s64, bound, ri, rs, sure = CR.fp64_reference(prec, emb, cand, lists, k)
    assert sure.shape == (64, k) and sure.mean() >= 0.95, sure.mean()
    assert 0.45 < (cand != 0).mean() < 0.55 and cand[ri[ri != 0]].all()


# ------------------------------------------------------------------ the text entry point
def test_text_runner_recommend_with_candidate_items(tmp_path, monkeypatch):
    """train one epoch through run.py, then --mode recommend --candidate_items from its checkpoint: every recommended item is a candidate, no
    seen item is returned, and the lists are the unrestricted run's with the non-candidates struck out (where that leaves topk of them)."""
    import test_text_run as TR
    import test_topk_cpu as TC
    TC._simulated(monkeypatch)
    monkeypatch.setattr(sim_lib, 'topk_items_cand', sim_topk_items_cand, raising=False)
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'cand']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    news = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    _, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), {n: i + 1 for i, n in enumerate(news)}, 20, 5)
    names = item_names[1:]                                                        # the items the reader keeps, by the names it writes
    stock = set(names[::3])
    cfile = os.path.join(root, 'stock.txt')
    with open(cfile, 'w') as f:
        f.write('\n'.join(sorted(stock)) + '\n\n' + names[0] + '\n')
    full, masked = os.path.join(root, 'full.tsv'), os.path.join(root, 'masked.tsv')
    rec = ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5']
    TR._run(common + rec + ['--recommend_out', full, '--topk', str(len(names))], monkeypatch, dict(loss=[], batch=[], eval=[]))
    TR._run(common + rec + ['--recommend_out', masked, '--candidate_items', cfile], monkeypatch, dict(loss=[], batch=[], eval=[]))
    a = [l.rstrip('\n').split('\t') for l in open(full)]
    b = [l.rstrip('\n').split('\t') for l in open(masked)]
    assert [x[0] for x in a] == [x[0] for x in b] and len(b) > 0
    some = 0
    for (_, items_a, _), (_, items_b, scores_b) in zip(a, b):
        got = items_b.split(' ') if items_b else []
        assert set(got) <= stock
        want = [x for x in items_a.split(' ') if x in stock][:5]
        assert got == want and len(scores_b.split(' ') if scores_b else []) == len(got)
        some += len(got)
    assert some > 0
    # --mode test with the same file: both splits ranked within the set, `k of n users` beside each metrics line (TR._run's recorder stands in
    # for run_eval_once with the unrestricted argument list, so this run goes through run.main itself)
    import logging
    import socket
    import torch.distributed as dist
    from adapter4rec_amd import run
    monkeypatch.setattr(sim_lib, 'eval_rank_cand', sim_eval_rank_cand, raising=False)
    monkeypatch.setattr(sim_lib, 'eval_rank', _refuse)
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    for k, v in dict(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE='1', RANK='0', LOCAL_RANK='0').items():
        monkeypatch.setenv(k, v)
    seen = []

    class Keep(logging.Handler):
        def emit(self, record):
            seen.append(record.getMessage())
    keep = Keep()
    logging.getLogger('Log_file').addHandler(keep)
    try:
        run.main(common + ['--mode', 'test', '--load_ckpt_name', 'epoch-1.pt', '--candidate_items', cfile])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        for name in ('Log_file', 'Log_screen'):
            lg = logging.getLogger(name)
            for h in list(lg.handlers):
                lg.removeHandler(h)
                h.close()
    assert any(l.startswith('candidate items: %d of ' % len(stock)) for l in seen), seen[-12:]
    for split in ('valid', 'test'):
        line = [l for l in seen if l.startswith(split + '_candidates')]
        assert len(line) == 1 and re.search(r'(\d+) of (\d+) users', line[0]), seen[-12:]
        k_users, n_users = map(int, re.search(r'(\d+) of (\d+) users', line[0]).groups())
        assert 0 < k_users < n_users == len(b)
    assert sum(c[0] == 'rank' for c in CALLS) >= 2
