"""a4r_topk_items on the MI355X (include/a4r.h): exact lists against a lexsort oracle, random tables against fp64, agreement with a4r_eval_rank,
determinism across grids, argument errors; recommend() against the CPU oracle's user tower; HR@10 from recommend() = eval_model's; the text
entry point's --mode recommend file against the oracle."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch

from topk_ref import csr, topk_reference, trigger_case, trigger_expected

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def run_topk(prec, emb, lists, k):
    from adapter4rec_amd import _lib as L
    ptr, flat = csr(lists)
    U = prec.shape[0]
    ids = torch.empty(U, k, dtype=torch.int32, device=DEV)
    sc = torch.empty(U, k, dtype=torch.float32, device=DEV)
    L.topk_items(prec, emb, torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), k, ids, sc)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def excl_lists(rng, U, N1):
    """0 ids, 264 ids with repeats, pad / negative / out-of-range ids, everything in between."""
    out = []
    for u in range(U):
        n = (0, 264, int(rng.integers(1, 40)))[u % 3]
        x = rng.integers(-3, N1 + 5, size=n)
        if n:
            x[: n // 4] = x[n // 4: 2 * (n // 4)]                    # repeats
            x[-1] = 0
        out.append(x)
    return out


def oracle_exact(prec, emb, lists, k):
    """integer-valued tables: every score is exact in fp32; the fp64 product on the device is the same number."""
    U = prec.shape[0]
    s = (prec.double() @ emb.double().t())
    ids = np.zeros((U, k), np.int64)
    out = np.full((U, k), -np.inf, np.float32)
    for u in range(U):
        row = s[u].clone()
        row[0] = -np.inf
        ex = torch.as_tensor(np.asarray(lists[u], np.int64))
        ex = ex[(ex > 0) & (ex < row.numel())]
        row[ex.to(DEV)] = -np.inf
        v, i = torch.sort(row, descending=True, stable=True)         # stable: equal scores keep ascending ids
        v, i = v[:k].cpu().numpy(), i[:k].cpu().numpy()
        ok = np.isfinite(v)
        n = int(ok.sum())
        ids[u, :n], out[u, :n] = i[:n], v[:n]
    out[out == 0] = 0.0
    return ids, out


CASES = [  # (K, E, N1, U): every listed K, E, N1 and U at least once; short lists where N1 - 1 - |excl| < K
    (1, 64, 2, 1), (7, 128, 17, 15), (10, 64, 14720, 16), (64, 256, 65537, 17), (100, 512, 14720, 17), (256, 64, 500000, 16),
    (10, 64, 65537, 4096), (100, 128, 14720, 4096), (256, 512, 17, 16), (7, 64, 500000, 1), (256, 128, 65537, 15), (64, 64, 2, 17),
    (1, 256, 65537, 4096), (256, 64, 14720, 4096),
]


@pytest.mark.parametrize('K,E,N1,U', CASES)
def test_topk_exact_on_integer_tables(K, E, N1, U):
    rng = np.random.default_rng(K * 7 + E + N1 + U)
    emb = torch.from_numpy(rng.integers(-8, 9, size=(N1, E)).astype(np.float32))
    if N1 > 8:
        src = rng.integers(1, N1, size=N1 // 8)
        emb[rng.integers(1, N1, size=N1 // 8)] = emb[src]             # duplicated rows: equal scores, ties broken by id
    prec = torch.from_numpy(rng.integers(-8, 9, size=(U, E)).astype(np.float32))
    prec[::5] = 0.0                                                  # every score 0: the list is the smallest candidate ids
    prec, emb = prec.to(DEV), emb.to(DEV)
    lists = excl_lists(rng, U, N1)
    ids, sc = run_topk(prec, emb, lists, K)
    ri, rs = oracle_exact(prec, emb, lists, K)
    np.testing.assert_array_equal(ids, ri)
    np.testing.assert_array_equal(sc.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize('K,E', [(64, 64), (256, 64)])                # cap = 128: a step's 64 keys fill the buffer, compaction at every step; cap = 512
def test_topk_exact_with_every_column_appended_at_every_step(K, E):
    """topk_ref.trigger_case: the append, the trigger and the compaction at the bound of 64 keys per user and step"""
    emb, prec, lists = trigger_case(E)
    ri, rs = trigger_expected(emb, prec, lists, K)
    ids, sc = run_topk(torch.from_numpy(prec).to(DEV), torch.from_numpy(emb).to(DEV), [lists[u % 3] for u in range(prec.shape[0])], K)
    np.testing.assert_array_equal(ids, ri)
    np.testing.assert_array_equal(sc.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize('K,E', [(10, 64), (100, 128), (256, 512)])
def test_topk_random_tables_against_fp64(K, E):
    rng = np.random.default_rng(K + E)
    U, N1 = 64, 65537
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    prec = torch.from_numpy(rng.standard_normal((U, E)).astype(np.float32)).to(DEV)
    lists = excl_lists(rng, U, N1)
    ids, sc = run_topk(prec, emb, lists, K)
    s64 = (prec.double() @ emb.double().t()).cpu().numpy()
    # fp32 summation of E products: |error| <= E * 2^-24 * sum |a b| (the classical recursive-summation bound).  The 2e-7 * sum |a b| first asked
    # for is met by typical items but not by the largest scores, whose partial sums are all large: measured up to 2.7e-7 (E = 64 .. 512)
    bound = E * 2.0 ** -24 * (prec.double().abs() @ emb.double().abs().t()).cpu().numpy()
    ri, rs = topk_reference(s64, lists, K + 1)
    for u in range(U):
        got = s64[u, ids[u]]
        assert np.all(np.abs(sc[u] - got) <= bound[u, ids[u]]), u
        b = bound[u].max()
        gap = np.diff(rs[u])                                          # <= 0: adjacent oracle gaps
        sep = np.concatenate([[True], -gap > b])                      # position j separated from j - 1 ...
        sure = sep[:K] & sep[1:K + 1]                                 # ... and from j + 1
        np.testing.assert_array_equal(ids[u][sure], ri[u][:K][sure])


def test_topk_agrees_with_eval_rank():
    from adapter4rec_amd import _lib as L
    rng = np.random.default_rng(3)
    U, N1, E, K = 4096, 65537, 64, 100
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    # users pointed at a few items so that many targets rank inside the list
    tgt = rng.integers(1, N1, size=U)
    prec = (emb[torch.from_numpy(tgt).to(DEV)] * 0.3 + torch.from_numpy(rng.standard_normal((U, E)).astype(np.float32)).to(DEV)).contiguous()
    hist = []
    for u in range(U):
        h = rng.integers(1, N1, size=int(rng.integers(1, 30)))
        hist.append(h[h != tgt[u]])
    ids, sc = run_topk(prec, emb, hist, K)
    ptr, flat = csr(hist)
    rank = torch.zeros(U, dtype=torch.int32, device=DEV)
    L.eval_rank(prec, emb, torch.from_numpy(tgt.astype(np.int32)).to(DEV), torch.from_numpy(ptr).to(DEV), torch.from_numpy(flat).to(DEV), rank)
    rank = rank.cpu().numpy()
    inside = 0
    for u in range(U):
        r = int(rank[u])
        if r <= K:
            inside += 1
            assert ids[u, r - 1] == tgt[u], (u, r)
            assert int((sc[u] > sc[u, r - 1]).sum()) == r - 1, u
        else:
            assert tgt[u] not in ids[u], u
    assert inside > U // 8, inside


def test_topk_deterministic_and_grid_independent():
    rng = np.random.default_rng(4)
    U, N1, E, K = 32768, 65537, 64, 100
    emb = torch.from_numpy(rng.standard_normal((N1, E)).astype(np.float32)).to(DEV)
    prec = torch.from_numpy(rng.standard_normal((U, E)).astype(np.float32)).to(DEV)
    lists = excl_lists(rng, U, N1)
    a = run_topk(prec, emb, lists, K)
    b = run_topk(prec, emb, lists, K)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for u in (0, 12345, U - 1):                                       # alone: 1 workgroup x 32 item ranges + the merge; in the batch: 1 range
        i1, s1 = run_topk(prec[u:u + 1].contiguous(), emb, [lists[u]], K)
        np.testing.assert_array_equal(i1[0], a[0][u])
        np.testing.assert_array_equal(s1[0].view(np.uint32), a[1][u].view(np.uint32))


def test_topk_argument_errors_launch_nothing():
    from adapter4rec_amd import _lib as L
    lib = L.lib()
    U, N1 = 16, 100
    emb = torch.randn(N1 + 1, 128, device=DEV)
    prec = torch.randn(U, 128, device=DEV)
    ptr = torch.zeros(U + 1, dtype=torch.int32, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids = torch.full((U, 257), 7, dtype=torch.int32, device=DEV)
    sc = torch.full((U, 257), 7.0, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    f = lib.a4r_topk_items
    assert (f.restype, f.argtypes) == L.SIGNATURES['a4r_topk_items']      # installed by lib()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    for args in ((prec, 0, emb, 0, 128, 0), (prec, 0, emb, 0, 128, 257), (prec, 0, emb, 0, 96, 10), (prec, 4, emb, 0, 64, 10), (prec, 0, emb, 4, 64, 10)):
        p, po, e, eo, E, K = args
        assert f(None, P(p, po), P(e, eo), P(ptr), P(idx), P(ids), P(sc), P(ws), U, N1, E, K) == -1, args
    assert L.topk_ws_bytes(U, N1, 0) == 0 and L.topk_ws_bytes(U, N1, 257) == 0
    torch.cuda.synchronize()
    assert bool((ids == 7).all()) and bool((sc == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ API and runner level

def _id_model():
    import test_id_tower_cpu as CPU
    model, fx, _ = CPU.build('sasrec', compute_dtype='fp32')
    args = CPU.make_args(arch='sasrec', adapter_type='None')
    return model.to(DEV), args, int(fx['item_num'])


def _oracle_lists(sd, emb, user_seqs, excl, k, T, arch='sasrec'):
    from oracle import ref_cpu as R
    cfg = dict(R.DEFAULT_CFG, arch=arch, max_seq_len=T, embedding_dim=emb.shape[1])
    sd64 = {n: v.double().cpu() for n, v in sd.items()}
    emb64 = emb.double().cpu()
    rows, bounds = [], []
    with torch.no_grad():
        for u in range(len(user_seqs)):
            toks = list(user_seqs[u])[-T:]
            ids = [0] * (T - len(toks)) + toks
            mask = torch.tensor([[0.0] * (T - len(toks)) + [1.0] * len(toks)], dtype=torch.float64)
            prec = R.user_encoder(sd64, emb64[ids][None], mask, cfg)[0, -1]
            rows.append((emb64 @ prec).numpy())
            bounds.append((emb64.abs() @ prec.abs()).numpy())
    ri, rs = topk_reference(np.stack(rows), excl, k + 1)
    return ri, rs, np.stack(bounds)


def _assert_gap_rule(ids, ri, rs, bound, tol):
    k = ids.shape[1]
    for u in range(ids.shape[0]):
        b = tol * bound[u].max()
        sep = np.concatenate([[True], -np.diff(rs[u]) > b])
        sure = sep[:k] & sep[1:k + 1]
        np.testing.assert_array_equal(ids[u][sure], ri[u][:k][sure])
        assert sure.mean() > 0.5, u


def test_recommend_id_tower_against_oracle():
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import recommend
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    rng = np.random.default_rng(6)
    seqs = {u: list(rng.integers(1, item_num + 1, size=int(rng.integers(1, 30)))) for u in range(37)}
    k = 10
    ids, sc = recommend(model, seqs, emb, k, args)
    ri, rs, bound = _oracle_lists(model.state_dict(), emb, seqs, [seqs[u] for u in range(37)], k, args.max_seq_len)
    _assert_gap_rule(ids.cpu().numpy(), ri, rs, bound, 1e-5)
    np.testing.assert_allclose(sc.cpu().numpy(), rs[:, :k], rtol=0, atol=1e-5 * bound.max())


def test_recommend_hr10_equals_eval_model():
    from adapter4rec_amd.cv.data_utils import get_itemId_embeddings
    from adapter4rec_amd.data_utils.metrics import eval_model, recommend
    model, args, item_num = _id_model()
    emb = get_itemId_embeddings(model, item_num, 256, args, 0)
    rng = np.random.default_rng(7)
    U = 300
    eval_seq, hist = {}, {}
    for u in range(U):
        s = list(rng.choice(np.arange(1, item_num + 1), size=int(rng.integers(3, args.max_seq_len + 2)), replace=False))
        eval_seq[u] = s
        hist[u] = torch.LongTensor(np.array(s[:-1]))
    hr = eval_model(model, hist, eval_seq, emb, 256, args, item_num, logging.getLogger('t'), 'test', 0)
    ids, _ = recommend(model, {u: eval_seq[u][:-1] for u in range(U)}, emb, 10, args, exclude=hist)
    ids = ids.cpu().numpy()
    hits = int(sum(eval_seq[u][-1] in ids[u] for u in range(U)))
    assert hits == round(hr * U) and abs(hits / U - hr) < 1e-6, (hits, hr)


def test_text_runner_recommend_matches_oracle(tmp_path, monkeypatch):
    import test_topk_cpu as TC
    TC.text_recommend_flow(tmp_path, monkeypatch, tol=1e-5)
