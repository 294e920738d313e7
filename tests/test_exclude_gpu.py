"""a4r_topk_items_excl on the MI355X (include/a4r_exclude.h): the bits of a4r_topk_items / a4r_topk_items_cand on the lists both entries serve,
exact lists against the restatement (tests/exclude_ref.py) on lists far beyond the 264-id cap, neighbouring lists, the compaction trigger, float
tables against a4r_topk_items on the table with the listed rows removed, determinism across grids; recommend(exclude_lists=...) on the ID model
and --mode recommend --exclude_history full --exclude_lists through the image entry point."""
import glob
import logging
import os
import re

import numpy as np
import pytest
import torch

import exclude_ref as XR
from test_topk_gpu import excl_lists
from topk_ref import csr as csr32, trigger_case, trigger_expected

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BITS = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return a.to(DEV) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_excl(prec, emb, lists, k, cand=None, csr=None):
    """prec / emb: device tensors; lists: per-user ids in any order (sorted here, as the contract asks) -> (ids, scores) numpy"""
    from adapter4rec_amd import _lib as L
    ptr, flat = XR.csr64(lists) if csr is None else csr
    U = prec.shape[0]
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    L.topk_items_excl(prec, emb, dev(ptr), dev(flat), None if cand is None else dev(cand), k, ids, sc)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def run_plain(prec, emb, lists, k, cand=None):
    """a4r_topk_items / a4r_topk_items_cand on the same lists (as they come: that kernel sorts them itself)"""
    from adapter4rec_amd import _lib as L
    ptr, flat = csr32(lists)
    U = prec.shape[0]
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    if cand is None:
        L.topk_items(prec, emb, dev(ptr), dev(flat), k, ids, sc)
    else:
        L.topk_items_cand(prec, emb, dev(ptr), dev(flat), dev(cand), k, ids, sc)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def assert_exact(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(BITS(got[1]), BITS(want[1]))


# ------------------------------------------------------------------ the bits of the existing entries
@pytest.mark.parametrize('E', (64, 128, 256, 512))
@pytest.mark.parametrize('U,N1,K', [(17, 4099, 10), (33, 14720, 100), (16, 1025, 256)])
def test_excl_has_the_bits_of_topk_items_and_topk_items_cand(E, U, N1, K):
    rng = np.random.default_rng(E + U + K)
    emb = dev(rng.standard_normal((N1, E)).astype(np.float32))
    prec = dev(rng.standard_normal((U, E)).astype(np.float32))
    lists = excl_lists(rng, U, N1)                                                 # empty, 264 ids with repeats, ids that are 0, negative or >= N1
    assert {len(l) for l in lists} >= {0, 264} and any((l <= 0).any() for l in lists if len(l))
    same = lambda a, b: torch.equal(torch.from_numpy(a[0]), torch.from_numpy(b[0])) and torch.equal(torch.from_numpy(a[1]).view(torch.int32), torch.from_numpy(b[1]).view(torch.int32))
    assert same(run_excl(prec, emb, lists, K), run_plain(prec, emb, lists, K))
    mask = (rng.random(N1) < 0.1).astype(np.uint8)
    got = run_excl(prec, emb, lists, K, mask)
    assert same(got, run_plain(prec, emb, lists, K, mask))
    assert mask[got[0][got[0] != 0]].all()


# ------------------------------------------------------------------ long lists, exact
def integer_case(rng, U, N1, E):
    emb = rng.integers(-8, 9, size=(N1, E)).astype(np.float32)
    if N1 > 8:
        emb[rng.integers(1, N1, size=N1 // 8)] = emb[rng.integers(1, N1, size=N1 // 8)]      # duplicated rows: equal scores, ties broken by id
    prec = rng.integers(-8, 9, size=(U, E)).astype(np.float32)
    prec[::5] = 0.0                                                                # every score 0: the list is the smallest candidate ids
    s = (prec.astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32)    # exact: integers far below 2^24
    return emb, prec, s


def best_items(s_row, n):
    """the n best items 1 .. N1-1 of a score row in key order: score descending, ties by smaller id"""
    c = np.arange(1, s_row.size)
    return c[np.lexsort((c, -s_row[1:].astype(np.float64)))][:n]


def long_lists(rng, s, first_kind):
    """One list per user, the kinds in turn: 265 ids (with repeats and ids that are no item), 1 000 ids, N1 - 1 - 3 distinct items (three are
    left: pads follow), all of 1 .. N1-1 (pads only), exactly the user's 300 best items (every early key that beats the threshold is listed)."""
    U, N1 = s.shape
    out = []
    for u in range(U):
        kind = (u + first_kind) % 5
        if kind == 0:
            x = rng.integers(-3, N1 + 5, size=265)
        elif kind == 1:
            x = rng.integers(1, N1, size=1000)
        elif kind == 2:
            x = rng.permutation(np.arange(1, N1))[:max(N1 - 4, 0)]
        elif kind == 3:
            x = np.arange(1, N1)
        else:
            x = best_items(s[u], 300)
        out.append(x)
    return out


# (K, E, N1, U): K at the topk_cap edges (64 / 65: 128 -> 256 slots; 192 / 193: 256 -> 512), N1 one item, one tile and one more, a round of the
# four waves and one more, 32 ranges and the merge; U one user, a partial, a full and a second workgroup.  Every listed K, N1 and U occurs.
LONG_CASES = [(1, 64, 2, 1), (64, 512, 17, 15), (65, 64, 18, 16), (192, 512, 66, 17), (193, 64, 4099, 17), (256, 512, 4099, 16), (256, 64, 4099, 15),
              (64, 64, 4099, 17), (192, 64, 4099, 16), (1, 512, 4099, 17)]


@pytest.mark.parametrize('case,K,E,N1,U', [(i,) + c for i, c in enumerate(LONG_CASES)])
def test_excl_exact_on_integer_tables_with_long_lists(case, K, E, N1, U):
    rng = np.random.default_rng(K * 7 + E + N1 + U)
    emb, prec, s = integer_case(rng, U, N1, E)
    lists = long_lists(rng, s, case)
    got = run_excl(dev(prec), dev(emb), lists, K)
    want = XR.excl_reference(s, lists, K)
    assert_exact(got, want)
    for u, l in enumerate(lists):
        assert not set(got[0][u][got[0][u] != 0]) & set(np.asarray(l).tolist()), u
    mask = (rng.random(N1) < 0.5).astype(np.uint8)
    assert_exact(run_excl(dev(prec), dev(emb), lists, K, mask), XR.excl_reference(s, lists, K, mask))


def test_long_cases_cover_what_they_claim():
    assert {c[0] for c in LONG_CASES} == {1, 64, 65, 192, 193, 256} and {c[2] for c in LONG_CASES} == {2, 17, 18, 66, 4099}
    assert {c[3] for c in LONG_CASES} == {1, 15, 16, 17} and {c[1] for c in LONG_CASES} == {64, 512}
    kinds = {(u + i) % 5 for i, c in enumerate(LONG_CASES) if c[2] == 4099 for u in range(c[3])}
    assert kinds == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------ neighbouring lists
def test_excl_neighbouring_lists_do_not_leak():
    """Items 5 and 6 are every user's two best.  User u lists {5}, user u + 1 lists {6} -- as neighbours inside a workgroup (0, 1) and across
    two (15, 16): u lists 6 first and never 5, u + 1 lists 5 first and never 6.  User 8 has an empty list between two lists of 1 000 ids that
    hold 5 and 6: it lists both."""
    rng = np.random.default_rng(5)
    U, N1, E, K = 19, 1200, 64, 10
    emb, prec, _ = integer_case(rng, U, N1, E)
    prec[:, 0], emb[:, 0] = 8, 0
    emb[5], emb[6] = 0, 0
    emb[5, 0], emb[6, 0] = 2000, 1500                                              # 16 000 and 12 000: above anything the other columns give (<= 63 * 64)
    prec[::5] = 0
    prec[[0, 1, 15, 16, 8], 0] = 8                                                 # (none of these is a zero user)
    prec[[0, 15], 1:] = prec[1, 1:]
    s = (prec.astype(np.float64) @ emb.astype(np.float64).T).astype(np.float32)
    lists = [rng.integers(7, N1, size=300) for _ in range(U)]
    lists[0], lists[1], lists[15], lists[16] = [5], [6], [5], [6]
    lists[7] = np.concatenate([rng.integers(7, N1, size=998), [5, 6]])
    lists[8] = []
    lists[9] = np.concatenate([rng.integers(7, N1, size=998), [5, 6]])
    got = run_excl(dev(prec), dev(emb), lists, K)
    assert_exact(got, XR.excl_reference(s, lists, K))
    ids = got[0]
    for a in (0, 15):
        assert ids[a, 0] == 6 and 5 not in ids[a] and ids[a + 1, 0] == 5 and 6 not in ids[a + 1]
    assert ids[8, :2].tolist() == [5, 6] and not {5, 6} & set(ids[7]) and not {5, 6} & set(ids[9])
    assert_exact((got[0][8:9], got[1][8:9]), run_plain(dev(prec[8:9]), dev(emb), [[]], K))


# ------------------------------------------------------------------ the compaction trigger
@pytest.mark.parametrize('K', (64, 256))                                           # cap = 128: a compaction at every step; cap = 512
def test_excl_exact_with_every_column_appended_at_every_step(K):
    emb, prec, lists = trigger_case(64)
    ri, rs = trigger_expected(emb, prec, lists, K)
    U = prec.shape[0]
    rows = [np.sort(np.asarray(l, np.int64)) for l in lists]                       # the three classes' lists, ascending, laid out user by user
    lens = np.array([rows[u % 3].size for u in range(U)], np.int64)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate([np.concatenate(rows)] * (U // 3) + [rows[u % 3] for u in range(U - U % 3, U)] + [np.zeros(1, np.int64)]).astype(np.int32)
    assert flat.size == ptr[-1] + 1
    assert_exact(run_excl(dev(prec), dev(emb), None, K, csr=(ptr, flat)), (ri, rs))


# ------------------------------------------------------------------ long lists on float tables, exact without a tolerance
@pytest.mark.parametrize('E,K', [(64, 100), (256, 10)])
def test_excl_equals_topk_items_on_the_table_without_the_listed_rows(E, K):
    """A score depends on its two rows only, and the map from the shortened table's rows back to ids is monotone, so ties keep their order: the
    list must have the bits a4r_topk_items gives with an empty list on the table with the listed rows removed."""
    rng = np.random.default_rng(E + K)
    N1, U = 3001, 8
    emb_np = rng.standard_normal((N1, E)).astype(np.float32)
    emb_np[rng.integers(1, N1, size=200)] = emb_np[rng.integers(1, N1, size=200)]  # equal rows: ties
    emb, prec = dev(emb_np), dev(rng.standard_normal((U, E)).astype(np.float32))
    for u in range(U):
        listed = rng.choice(np.arange(1, N1), size=1500, replace=False)
        keep = np.setdiff1d(np.arange(N1), listed)                                 # ascending, row 0 first
        p = prec[u:u + 1].contiguous()
        got = run_excl(p, emb, [listed], K)
        i2, s2 = run_plain(p, emb[dev(keep)].contiguous(), [[]], K)
        assert_exact(got, (keep[i2], s2))
        assert not set(got[0][0]) & set(listed.tolist()) and (got[0] != 0).all()


# ------------------------------------------------------------------ grid independence
def test_excl_deterministic_and_grid_independent():
    """32 768 users are one item range, their first 4 096 alone eight, one user alone 32 ranges and the merge: the same lists, bit for bit."""
    rng = np.random.default_rng(4)
    U, N1, E, K, L_ = 32768, 14720, 64, 100, 300
    emb = dev(rng.standard_normal((N1, E)).astype(np.float32))
    prec = dev(rng.standard_normal((U, E)).astype(np.float32))
    pool = np.sort(rng.integers(1, N1, size=(64, L_)), axis=1)                     # user u has list u % 64
    flat = np.concatenate([np.tile(pool, (U // 64, 1)).ravel(), [0]]).astype(np.int32)
    ptr = np.arange(U + 1, dtype=np.int64) * L_
    a = run_excl(prec, emb, None, K, csr=(ptr, flat))
    assert_exact(run_excl(prec, emb, None, K, csr=(ptr, flat)), a)
    b = run_excl(prec[:4096].contiguous(), emb, None, K, csr=(ptr[:4097], flat))
    assert_exact(b, (a[0][:4096], a[1][:4096]))
    for u in (0, 2345, 4095):
        one = run_excl(prec[u:u + 1].contiguous(), emb, [pool[u % 64]], K)
        assert_exact(one, (a[0][u:u + 1], a[1][u:u + 1]))
        assert not set(one[0][0]) & set(pool[u % 64].tolist())


def test_excl_argument_errors_launch_nothing():
    import ctypes as C
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    U, N1 = 16, 101
    emb, prec = torch.randn(N1, 128, device=DEV), torch.randn(U, 128, device=DEV)
    ptr = torch.zeros(U + 2, dtype=torch.int64, device=DEV)
    flat = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = torch.full((U, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, 257), 7.0, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    f = lib.a4r_topk_items_excl
    assert (f.restype, f.argtypes) == L.EXCLUDE_SIGNATURES['a4r_topk_items_excl']
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    # (prec offset, emb offset, ws offset, ptr offset, U, N1, E, K)
    for po, eo, wo, xo, u, n1, E, K in ((0, 0, 0, 0, U, N1, 128, 0), (0, 0, 0, 0, U, N1, 128, 257), (0, 0, 0, 0, U, N1, 96, 10), (4, 0, 0, 0, U, N1, 64, 10),
                                        (0, 8, 0, 0, U, N1, 64, 10), (0, 0, 4, 0, U, N1, 64, 10), (0, 0, 0, 4, U, N1, 64, 10), (0, 0, 0, 0, 0, N1, 64, 10),
                                        (0, 0, 0, 0, U, 1, 64, 10)):
        assert f(None, P(prec, po), P(emb, eo), P(ptr, xo), P(flat), None, P(ids), P(sc), P(ws, wo), u, n1, E, K) == -1, (po, eo, wo, xo, u, n1, E, K)
    for null in (1, 2, 3, 4, 6, 7, 8):
        a = [None, P(prec), P(emb), P(ptr), P(flat), None, P(ids), P(sc), P(ws), U, N1, 128, 10]
        a[null] = None
        assert f(*a) == -1, null
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ API and runner level
def _id_model():
    from test_topk_gpu import _id_model as fixture
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    model, args, item_num = fixture()
    return model, args, item_num, get_itemId_embeddings(model, item_num, 256, args, 0)


def test_recommend_with_exclude_lists_on_the_id_model(monkeypatch):
    from adapter4rec_amd.data_utils.metrics import Diversify, recommend
    model, args, item_num, emb = _id_model()
    rng = np.random.default_rng(6)
    n, k = 37, 10
    seqs = {u: [int(x) for x in rng.integers(1, item_num + 1, size=int(rng.integers(1, 30)))] for u in range(n)}
    monkeypatch.setenv('A4R_EVAL_USER_BATCH', '16')                                # three batches: the offsets are sliced, not rebuilt
    plain_i, plain_s = recommend(model, seqs, emb, k, args)
    lists = {u: rng.integers(-5, item_num + 50, size=1000).tolist() for u in range(0, n, 2)}      # far beyond 264 ids, with ids that are no item
    lists[1] = []
    lists[3] = plain_i[3].tolist()                                                 # exactly what the plain call recommends
    lists[5] = set(range(1, item_num + 1))                                         # everything: pads only
    ids, sc = recommend(model, seqs, emb, k, args, exclude_lists=lists)
    assert ids.dtype == torch.long and tuple(ids.shape) == (n, k) == tuple(sc.shape)
    for u in range(n):
        got = set(ids[u].tolist()) - {0}
        assert not got & set(lists.get(u, ())) and not got & set(seqs[u]), u
        if u % 2 and u not in (3, 5):                                              # an empty list, or none: the plain call, bit for bit
            assert torch.equal(ids[u], plain_i[u]) and torch.equal(sc[u], plain_s[u]), u
    assert (ids[5] == 0).all() and torch.isneginf(sc[5]).all() and not set(ids[3].tolist()) & set(plain_i[3].tolist())
    left = [item_num - len(set(lists[u]) & set(range(1, item_num + 1)) | set(seqs[u])) for u in range(0, n, 2)]
    assert [int((ids[u] != 0).sum()) for u in range(0, n, 2)] == [min(k, x) for x in left]
    mask = np.zeros(item_num + 1, bool)
    mask[rng.choice(np.arange(1, item_num + 1), size=item_num // 2, replace=False)] = True
    ci, _ = recommend(model, seqs, emb, k, args, exclude_lists=lists, candidates=mask)
    for u in range(n):
        got = set(ci[u].tolist()) - {0}
        assert mask[list(got)].all() and not got & set(lists.get(u, ())) and not got & set(seqs[u]), u
    di, _ = recommend(model, seqs, emb, 5, args, exclude_lists=lists, diversify=Diversify(0.5, 20))
    pool, _ = recommend(model, seqs, emb, 20, args, exclude_lists=lists)
    for u in range(n):
        assert set(di[u].tolist()) - {0} <= set(pool[u].tolist()) - {0}, u
    with pytest.raises(ValueError, match='candidate_lists'):
        recommend(model, seqs, emb, k, args, exclude_lists=lists, candidate_lists={0: [1, 2]})
    with pytest.raises(ValueError, match='bf16'):
        recommend(model, seqs, emb, k, args, exclude_lists=lists, score_dtype='bf16')


def test_cv_id_runner_recommend_with_exclude_flags(tmp_path, monkeypatch):
    """The image entry point with --item_tower id on the GPU: one epoch, then --mode recommend --exclude_history full --exclude_lists f.tsv from
    its checkpoint: no line holds an item of the user's whole line of the behaviours file or of the user's list in f.tsv, and the counts are logged."""
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.data_utils import read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    orig_setup = RA.setuplogger

    def setup(*a, **kw):                                                          # (_run_cv drops the loggers' handlers after every run)
        out = orig_setup(*a, **kw)
        logging.getLogger('Log_file').addHandler(Keep())
        return out
    monkeypatch.setattr(RA, 'setuplogger', setup)
    behaviours = os.path.join(data, 'toy', 'users_log.tsv')
    _, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    user_names, item_names = read_behavior_names(behaviours, name2id, 20, 5)
    full = {}
    for l in open(behaviours):
        name, seq = l.rstrip('\n').split('\t')[:2]
        full[name] = set(seq.split(' '))
    assert any(len(v) > 23 for v in full.values())                                 # some lines are longer than the reader's window
    plain = os.path.join(root, 'plain.tsv')
    rec = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--recommend_out', plain], monkeypatch, rec)
    first = {l.split('\t')[0]: l.rstrip('\n').split('\t')[1].split(' ') for l in open(plain)}
    blocked = {u: first[u][:2] for u in user_names[::2]}                           # block what the plain run recommends first
    f = os.path.join(root, 'f.tsv')
    with open(f, 'w') as fh:
        for u, items in blocked.items():
            fh.write(u + '\t' + ' '.join(items + ['gone_item']) + '\n')
        fh.write('nobody\tv1 v2\n')
    out = os.path.join(root, 'rec.tsv')
    CR._run_cv(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--recommend_out', out, '--exclude_history', 'full',
                         '--exclude_lists', f], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == []
    rows = [l.rstrip('\n').split('\t') for l in open(out)]
    assert [r[0] for r in rows] == user_names
    changed = 0
    for name, items, scores in rows:
        items = items.split(' ')
        assert 1 <= len(items) <= 5 and not set(items) & full[name] and not set(items) & set(blocked.get(name, ())), name
        assert set(items) <= set(item_names[1:])
        changed += items != first[name]
    assert changed >= len(blocked)
    line = [l for l in lines if l.startswith('exclude lists: ')]
    assert len(line) == 1
    m = re.fullmatch(r'exclude lists: (\d+) users, (\d+) ids in all, longest (\d+); (\d+) user names and (\d+) item names unknown, skipped <- (.*)', line[0])
    known = set(item_names[1:])
    want = {u: (full[u] & known) | set(blocked.get(u, ())) for u in user_names}
    assert m and [int(x) for x in m.groups()[:5]] == [len(user_names), sum(len(v) for v in want.values()), max(len(v) for v in want.values()),
                                                      1 + len(set(full) - set(user_names)), 1 + len(set().union(*full.values()) - known - {''})]
    assert m.group(6).endswith(f) and '--exclude_history full' in m.group(6)
