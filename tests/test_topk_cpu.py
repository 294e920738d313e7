"""CPU side of top-K recommendation (include/a4r.h: a4r_topk_items): ABI version and exports, argument checks before any launch, the binding's
validation, the behaviours-file name recovery, and --mode recommend through both entry points on the simulated library (tests/sim_lib.py plus
the numpy restatement in tests/topk_ref.py), against the CPU oracle."""
import ctypes
import glob
import json
import logging
import os

import numpy as np
import pytest
import torch

import sim_lib
from topk_ref import sim_topk_items, topk_reference


def test_abi_411_and_topk_exports():
    from adapter4rec_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    assert L.ABI_VERSION == 411 and lib.a4r_version() == 411
    assert hasattr(lib, 'a4r_topk_items') and hasattr(lib, 'a4r_topk_ws_bytes') and 'a4r_topk_items' in L.EXPORTS
    # workspace: one K-key list per user and item range (a host query)
    assert L.topk_ws_bytes(32768, 65537, 10) == 32768 * 10 * 8
    assert L.topk_ws_bytes(1, 500000, 256) == 32 * 256 * 8
    assert L.topk_ws_bytes(16, 2, 7) == 16 * 7 * 8
    for bad in ((0, 100, 10), (16, 1, 10), (16, 100, 0), (16, 100, 257)):
        assert L.topk_ws_bytes(*bad) == 0, bad


def test_topk_null_and_shape_probes_return_einval():
    from adapter4rec_amd import _lib as L
    if torch.cuda.is_available():
        pytest.skip('argument-check probe is a CPU test')
    f = ctypes.CDLL(L.LIB_PATH).a4r_topk_items
    f.restype, f.argtypes = L.SIGNATURES['a4r_topk_items']
    assert f(*([None] * 8), 0, 0, 0, 0) == -1
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p16 = (p + 15) // 16 * 16
    ok = [None, p16, p16, p16, p16, p16, p16, p16]
    for U, N1, E, K in ((16, 100, 64, 0), (16, 100, 64, 257), (16, 100, 96, 10), (0, 100, 64, 10), (16, 1, 64, 10)):
        assert f(*ok, U, N1, E, K) == -1, (U, N1, E, K)
    assert f(None, p16 + 4, p16, p16, p16, p16, p16, p16, 16, 100, 64, 10) == -1          # misaligned prec
    assert f(None, p16, p16 + 4, p16, p16, p16, p16, p16, 16, 100, 64, 10) == -1          # misaligned item table


def test_binding_validates_before_the_library():
    from adapter4rec_amd import _lib as L
    with pytest.raises(RuntimeError, match='device tensors'):
        L.topk_items(torch.zeros(4, 64), torch.zeros(9, 64), torch.zeros(5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3,
                     torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3))
    orig = L.require_gpu
    try:
        L.require_gpu = lambda *t: None                                 # reach the shape checks on host tensors
        args = lambda **kw: dict(dict(prec=torch.zeros(4, 64), item_emb=torch.zeros(9, 64), excl_ptr=torch.zeros(5, dtype=torch.int32),
                                      excl_idx=torch.zeros(1, dtype=torch.int32), k=3, ids=torch.zeros(4, 3, dtype=torch.int32),
                                      scores=torch.zeros(4, 3)), **kw)
        for bad, msg in ((dict(k=0), 'outside'), (dict(k=257), 'outside'), (dict(prec=torch.zeros(4, 96), item_emb=torch.zeros(9, 96)), 'supported'),
                         (dict(item_emb=torch.zeros(9, 128)), 'expected'), (dict(prec=torch.zeros(4, 64, dtype=torch.float64)), 'fp32'),
                         (dict(excl_ptr=torch.zeros(4, dtype=torch.int32)), 'U \\+ 1'), (dict(ids=torch.zeros(4, 2, dtype=torch.int32)), 'must be'),
                         (dict(excl_idx=torch.zeros(1, dtype=torch.int64)), 'int32'), (dict(item_emb=torch.zeros(1, 64)), 'N1 >= 2')):
            with pytest.raises(ValueError, match=msg):
                L.topk_items(**args(**bad))
    finally:
        L.require_gpu = orig


def test_reference_semantics():
    """the restatement itself: ties by id, exclusions (repeats, 0, out of range), NaN last, short lists padded, -0 as +0"""
    s = np.array([[0.0, 1.0, 3.0, 3.0, np.nan, -0.0, 2.0]], np.float32)
    i, v = topk_reference(s, [[6, 6, 0, 99, -1]], 6)
    assert i.tolist() == [[2, 3, 1, 5, 4, 0]]
    assert v[0, :3].tolist() == [3.0, 3.0, 1.0] and np.signbit(v[0, 3]) == False and np.isnan(v[0, 4]) and v[0, 5] == -np.inf


def test_behavior_names_match_read_behaviors(tmp_path):
    from test_text_run import write_toy
    from adapter4rec_amd.data_utils import read_behaviors
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    data = write_toy(str(tmp_path))
    path = os.path.join(data, 'toy', 'behaviors.tsv')
    with open(path, 'a') as f:                                          # a short user (dropped) and a repeated user name (first place, last line)
        f.write('U999\tN1 N2\n')
        f.write('U3\t' + ' '.join(f'N{i}' for i in (5, 6, 7, 8, 9, 10)) + '\n')
    names = [l.split('\t')[0] for l in open(os.path.join(data, 'toy', 'news.tsv'))]
    before = {n: i + 1 for i, n in enumerate(names)}
    id2dic = {i + 1: n for i, n in enumerate(names)}
    item_num, id2dic2, tr, va, te, hv, ht = read_behaviors(path, id2dic, before, 20, 5, logging.getLogger('t'))
    users, items = read_behavior_names(path, before, 20, 5)
    assert len(users) == len(te) and 'U999' not in users and users[3] == 'U3' and len(items) == item_num + 1
    assert [items[i] for i in range(1, item_num + 1)] == [id2dic2[i] for i in range(1, item_num + 1)]      # the reader's renumbering
    last = {}
    for line in open(path):
        u, seq = line.rstrip('\n').split('\t')
        if len(seq.split(' ')) >= 5:
            last[u] = seq.split(' ')[-21:]
    for uid, name in enumerate(users):
        assert [items[i] for i in te[uid]] == last[name], name


# ------------------------------------------------------------------------------------------------------------------ entry points

def _simulated(monkeypatch):
    import test_text_run as TR
    TR._simulate(monkeypatch)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)


def text_recommend_flow(tmp_path, monkeypatch, tol):
    """train one epoch through run.py, then --mode recommend from its checkpoint; every line against the oracle's lists (item embeddings and user
    tower of oracle/ref_cpu.py on the saved weights, fp64 scores, the seen sequence excluded) up to the gap rule."""
    import test_text_run as TR
    from oracle import ref_cpu as R
    from transformers import BertTokenizer
    from adapter4rec_amd.data_utils import get_doc_input_bert, read_behaviors, read_news_bert
    from adapter4rec_amd.parameters import parse_args
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'rec']
    TR._run(common + ['--mode', 'train', '--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    rec = dict(loss=[], batch=[], eval=[])
    TR._run(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '7'], monkeypatch, rec)
    assert rec['loss'] == [] and rec['eval'] == []                      # no training step, no evaluation
    out = os.path.join(os.path.dirname(ck[0]), 'recommend_epoch-1.pt.tsv')
    lines = [l.rstrip('\n').split('\t') for l in open(out)]

    args = parse_args(['--num_words_title', '30'])
    tok = BertTokenizer.from_pretrained('../pretrained_models/bert/bert_tiny')
    news = os.path.join(data, 'toy', 'news.tsv')
    id2dic, name2id = read_news_bert(news, args, tok)
    item_num, id2dic2, tr, va, te, hv, ht = read_behaviors(os.path.join(data, 'toy', 'behaviors.tsv'), id2dic, name2id, 20, 5, logging.getLogger('t'))
    title, mask, *_ = get_doc_input_bert(id2dic2, args)
    content = np.concatenate([title, mask], axis=1).astype(np.int64)
    sd = {k: v.double() for k, v in torch.load(ck[0], map_location='cpu', weights_only=False)['model_state_dict'].items()}
    cfg = dict(R.DEFAULT_CFG, bert_heads=2)
    with torch.no_grad():
        emb = R.item_embeddings(sd, content, cfg).double()
        rows, bounds, excl = [], [], []
        for u in range(len(te)):
            toks = list(te[u])[-20:]
            ids = [0] * (20 - len(toks)) + toks
            m = torch.tensor([[0.0] * (20 - len(toks)) + [1.0] * len(toks)], dtype=torch.float64)
            prec = R.user_encoder(sd, emb[ids][None], m, cfg)[0, -1].double()
            rows.append((emb @ prec).numpy())
            bounds.append((emb.abs() @ prec.abs()).numpy())
            excl.append(list(ht[u].numpy()) + [te[u][-1]])
    ri, rs = topk_reference(np.stack(rows), excl, 8)
    user_names = []
    for l in open(os.path.join(data, 'toy', 'behaviors.tsv')):
        u, seq = l.rstrip('\n').split('\t')
        if len(seq.split(' ')) >= 5 and u not in user_names:
            user_names.append(u)
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    _, item_names = read_behavior_names(os.path.join(data, 'toy', 'behaviors.tsv'), name2id, 20, 5)
    assert [l[0] for l in lines] == user_names
    for u, (name, items, scores) in enumerate(lines):
        items, scores = items.split(' '), np.array([float(x) for x in scores.split(' ')])
        assert len(items) == len(scores) == 7
        b = tol * np.abs(bounds[u]).max()
        sep = np.concatenate([[True], -np.diff(rs[u]) > b])
        sure = sep[:7] & sep[1:8]
        want = [item_names[i] for i in ri[u][:7]]
        assert [x for x, s in zip(items, sure) if s] == [x for x, s in zip(want, sure) if s], name
        np.testing.assert_allclose(scores, rs[u][:7], rtol=0, atol=b + 1e-6)
        assert not set(items) & {item_names[i] for i in excl[u]}, name
    return out


def test_text_runner_recommend_simulated(tmp_path, monkeypatch):
    _simulated(monkeypatch)
    text_recommend_flow(tmp_path, monkeypatch, tol=1e-5)


def test_text_parser_recommend_flags():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.parameters import parse_args
    a = parse_args(['--mode', 'recommend'])
    assert a.mode == 'recommend' and a.topk == 10 and a.recommend_out is None
    b = cv_parse(['--mode', 'recommend', '--topk', '3', '--recommend_out', 'x.tsv'])
    assert b.topk == 3 and b.recommend_out == 'x.tsv'
    assert parse_args([]).mode == 'train'


def test_recommend_rejects_long_exclusion_lists():
    from adapter4rec_amd.data_utils.metrics import _recommend_inputs
    seqs = {0: [1, 2, 3], 1: [4]}
    with pytest.raises(ValueError, match='exceeds'):
        _recommend_inputs(seqs, {0: list(range(1, 266)), 1: [1]}, np.array([0, 1]), 5)
    ids, mask, ptr, flat = _recommend_inputs(seqs, None, np.array([0, 1]), 5)
    assert ids.tolist() == [[0, 0, 1, 2, 3], [0, 0, 0, 0, 4]] and mask.sum() == 4
    assert ptr.tolist() == [0, 3, 4] and flat.tolist() == [1, 2, 3, 4, 0]


def test_cv_id_runner_recommend_simulated(tmp_path, monkeypatch):
    """the image entry point with --item_tower id: train one epoch, --mode recommend from its checkpoint, every line = the CPU restatement's list
    (ID table + oracle user tower, fp64) up to the gap rule"""
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    from oracle import ref_cpu as R
    from adapter4rec_amd.cv.data_utils import read_behaviors, read_images
    from adapter4rec_amd.data_utils.preprocess import read_behavior_names
    IC_sim = [n for n in ('id_index', 'id_grad_sum', 'id_index_ws_ints') if hasattr(IC, n)]
    for n in IC_sim:
        monkeypatch.setattr(sim_lib, n, getattr(IC, n), raising=False)
    monkeypatch.setattr(sim_lib, 'topk_items', sim_topk_items, raising=False)
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS
    CR._run_cv(common + ['--epoch', '1'], monkeypatch, dict(loss=[], batch=[], eval=[]))
    ck = glob.glob(os.path.join(root, 'work', 'checkpoint_*', 'cpt_*', 'epoch-1.pt'))
    assert len(ck) == 1, ck
    out = os.path.join(root, 'rec.tsv')
    CR._run_cv(common + ['--mode', 'recommend', '--load_ckpt_name', 'epoch-1.pt', '--topk', '5', '--recommend_out', out], monkeypatch,
               dict(loss=[], batch=[], eval=[]))
    lines = [l.rstrip('\n').split('\t') for l in open(out)]
    keys, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    item_num, _, tr, va, te, hv, ht = read_behaviors(os.path.join(data, 'toy', 'users_log.tsv'), keys, name2id, 20, 5, logging.getLogger('t'))
    users, item_names = read_behavior_names(os.path.join(data, 'toy', 'users_log.tsv'), name2id, 20, 5)
    assert [l[0] for l in lines] == users
    sd = {k: v.double() for k, v in torch.load(ck[0], map_location='cpu', weights_only=False)['model_state_dict'].items()}
    emb = sd['id_embedding.weight']
    cfg = dict(R.DEFAULT_CFG, max_seq_len=20)
    for u, (name, items, scores) in enumerate(lines):
        toks = list(te[u])[-20:]
        ids = [0] * (20 - len(toks)) + toks
        m = torch.tensor([[0.0] * (20 - len(toks)) + [1.0] * len(toks)], dtype=torch.float64)
        with torch.no_grad():
            prec = R.user_encoder(sd, emb[ids][None], m, cfg)[0, -1]
        excl = list(ht[u].numpy()) + [te[u][-1]]
        ri, rs = topk_reference((emb @ prec).numpy()[None], [excl], 6)
        b = 1e-5 * float((emb.abs() @ prec.abs()).max())
        sep = np.concatenate([[True], -np.diff(rs[0]) > b])
        sure = sep[:5] & sep[1:6]
        got = items.split(' ')
        n = min(5, item_num - len(set(excl)))
        want = [item_names[i] for i in ri[0][:n]]
        assert len(got) == n
        assert [x for x, s in zip(got, sure) if s] == [x for x, s in zip(want, sure[:n]) if s], name
