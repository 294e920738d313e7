"""CPU: the ID item tower (--item_tower id, the reference's IDRec baseline: Downstream/CV/model/model.py with use_modal=False) -- model classes,
the engine's host logic through tests/sim_lib.py plus the two ID entry points restated below, data-parallel lock-step, flag checks, and the
image entry point end to end against a CPU restatement of the reference's evaluation.  The fixtures come from tools/gen_golden_r7.py."""
import argparse
import os

import numpy as np
import pytest
import torch

import id_fixture as F
import sim_lib

CHUNK = 16          # A4R_ID_SUM_CHUNK (include/a4r.h)


# ------------------------------------------------------------------ the two ID entry points, restated (include/a4r.h)
def id_index_ws_ints(n, item_num):
    assert 0 < n <= 1 << 20 and 0 < item_num < 2 ** 31 - 1
    return 1


CALLS = []


def id_index(ids, item_num, rows, slots, ptr, uniq, n_uniq, err, ws):
    CALLS.append('id_index')
    ids = ids.reshape(-1).long()
    n = ids.numel()
    ok = (ids >= 0) & (ids <= item_num)
    rows[:n] = torch.where(ok, ids, torch.zeros_like(ids)).to(torch.int32)
    err[0] = int((~ok).sum())
    key = torch.where(ok, ids, torch.zeros_like(ids)).numpy()
    order = np.argsort(key, kind='stable')
    slots[:n] = torch.from_numpy(order.astype(np.int32))
    sk = key[order]
    heads = np.flatnonzero((sk != 0) & np.concatenate([[True], sk[1:] != sk[:-1]]))
    uniq[:len(heads)] = torch.from_numpy(sk[heads].astype(np.int32))
    ptr[:len(heads)] = torch.from_numpy(heads.astype(np.int32))
    ptr[len(heads)] = n
    n_uniq[0] = len(heads)


def ordered_sum(src, lst):
    """S_r of include/a4r.h: chunks of CHUNK slots summed sequentially from 0.0f, the chunk sums added in chunk order (fp32 throughout)."""
    S = np.zeros(src.shape[1], np.float32)
    for c0 in range(0, len(lst), CHUNK):
        acc = np.zeros(src.shape[1], np.float32)
        for j in lst[c0:c0 + CHUNK]:
            acc = acc + src[j]
        S = S + acc
    return S


def id_grad_sum(src, slots, ptr, uniq, n_uniq, n, grad):
    CALLS.append('id_grad_sum')
    s = src.detach().numpy()
    sl, p = slots.numpy(), ptr.numpy()
    for u in range(int(n_uniq[0])):
        r = int(uniq[u])
        grad[r] = torch.from_numpy(grad[r].numpy() + ordered_sum(s, sl[p[u]:p[u + 1]]))


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.optim as O
    for name, f in (('id_index', id_index), ('id_grad_sum', id_grad_sum), ('id_index_ws_ints', id_index_ws_ints)):
        monkeypatch.setattr(sim_lib, name, f, raising=False)
    for mod in (E, EI, O):
        monkeypatch.setattr(mod, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    CALLS.clear()


def make_args(**kw):
    a = argparse.Namespace(max_seq_len=20, l2_weight=0, embedding_dim=64, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                           CV_model_load='vit-base-patch16-224', compute_dtype='fp32', arch='sasrec')
    for k, v in kw.items():
        setattr(a, k, v)
    return a


fixture = F.fixture
_REF = {}


def shapes_of(model):
    return {k: tuple(v.shape) for k, v in model.state_dict().items()}


def reference(arch):
    """The restated reference's step-1 gradients, losses and step-2 parameters (tests/id_fixture.py), pinned to the fixture by
    test_id_restatement_matches_the_reference_fixture."""
    if arch not in _REF:
        from adapter4rec_amd.cv import Model, ModelCPC
        m = (ModelCPC if arch == 'cpc' else Model)(make_args(arch=arch), F.ITEM_NUM, False)
        _REF[arch] = F.id_reference_step(arch, shapes_of(m))
    return _REF[arch]


def build(arch, **kw):
    """The model with the fixture's (derived) initial weights -> (model, fixture, restated reference)."""
    from adapter4rec_amd.cv import Model, ModelCPC
    fx = fixture(arch)
    model = (ModelCPC if arch == 'cpc' else Model)(make_args(arch=arch, **kw), int(fx['item_num']), False, None)
    model.load_state_dict(F.init_state(shapes_of(model)), strict=True)
    return model, fx, reference(arch)


def check_grads(model, ref, tol=1e-5):
    for k, p in model.named_parameters():
        want = ref['grad'][k]
        np.testing.assert_allclose(p.grad.detach().cpu().numpy(), want, atol=tol * max(np.abs(want).max(), 1e-30), rtol=0, err_msg=k)


@pytest.mark.parametrize('arch', ['sasrec', 'cpc'])
def test_id_restatement_matches_the_reference_fixture(arch):
    """The CPU restatement (oracle/ref_cpu.py user tower + head behind an ID lookup, torch autograd, torch.optim.Adam) reproduces what the
    imported reference stored: losses of both steps, the table / position / vector gradients, the matrix gradients' projections, the step-2
    table and vectors."""
    F.check_against_fixture(reference(arch), fixture(arch))


@pytest.mark.parametrize('arch', ['sasrec', 'cpc'])
def test_id_model_constructs_with_reference_keys(arch):
    from adapter4rec_amd.cv import Model, ModelCPC
    fx = fixture(arch)
    model = (ModelCPC if arch == 'cpc' else Model)(make_args(arch=arch), int(fx['item_num']), False)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in fx['keys']]
    for k in sd:                                                    # the shapes the reference's gradients had
        want = fx['grad/' + k].shape if 'grad/' + k in fx else (fx['gradproj_u/' + k].size, fx['gradproj_v/' + k].size)
        assert tuple(sd[k].shape) == want, k
    assert list(sd)[-1] == 'id_embedding.weight' and model.id_embedding.padding_idx == 0
    assert float(model.id_embedding.weight.detach()[0].abs().sum()) > 0            # xavier over every row, row 0 included (model.py:34-35)
    model.load_state_dict(F.init_state(shapes_of(model)), strict=True)


def test_text_model_keeps_refusing_the_id_tower():
    from adapter4rec_amd.model import Model
    with pytest.raises(NotImplementedError, match='is_use_modal'):
        Model(make_args(), 60, False, None)


@pytest.mark.parametrize('arch', ['sasrec', 'cpc'])
def test_id_host_logic_step_matches_reference(simulated, arch):
    model, fx, ref = build(arch)
    model.train()
    loss = model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 'cpu')
    loss.backward()
    assert abs(loss.item() - float(fx['loss1'])) <= 1e-5 * abs(float(fx['loss1']))
    check_grads(model, ref)
    g = model.id_embedding.weight.grad.numpy()
    touched = np.unique(fx['items1'])
    absent = np.setdiff1d(np.arange(g.shape[0]), touched[touched > 0])
    assert np.all(g[absent] == 0)
    assert CALLS.count('id_index') == 1 and CALLS.count('id_grad_sum') == 1


def test_id_host_logic_two_fused_adam_steps(simulated):
    """FusedAdam (flat buffers bound to the engine) over two batches against torch.optim.Adam in the reference (fixture)."""
    from adapter4rec_amd.optim import FusedAdam
    model, fx, ref = build('sasrec')
    model.train()
    opt = FusedAdam([{'params': list(model.parameters()), 'lr': 1e-3}])
    for step, (it, m) in enumerate((('items1', 'mask1'), ('items2', 'mask2')), 1):
        opt.zero_grad()
        loss = model(torch.from_numpy(fx[it]), torch.from_numpy(fx[m]), 'cpu')
        loss.backward()
        opt.step()
        assert abs(loss.item() - float(fx[f'loss{step}'])) <= 1e-5 * abs(float(fx[f'loss{step}']))
    w0, w = F.init_state(shapes_of(model))['id_embedding.weight'].numpy(), model.id_embedding.weight.detach().numpy()
    both = np.union1d(fx['items1'], fx['items2'])
    untouched = np.setdiff1d(np.arange(w.shape[0]), both[both > 0])
    assert 0 in untouched and np.array_equal(w[untouched], w0[untouched])
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.detach().numpy(), ref['step2'][k], atol=2e-5, rtol=0, err_msg=k)


def test_id_host_ids_out_of_range_raise_before_any_launch(simulated):
    model, fx, _ = build('sasrec')
    items = torch.from_numpy(fx['items1']).clone()
    for bad in (int(fx['item_num']) + 1, -1):
        items[3] = bad
        with pytest.raises(IndexError):
            model(items, torch.from_numpy(fx['mask1']), 'cpu')
    assert CALLS == []


def test_id_fp8_compute_dtype_refused(simulated):
    model, fx, _ = build('sasrec', compute_dtype='fp8')
    with pytest.raises(NotImplementedError, match='fp8'):
        model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 'cpu')


def test_id_encode_items_and_table(simulated):
    model, fx, _ = build('sasrec')
    eng = model._engine()
    ids = torch.tensor([0, 5, 60, 5])
    w0 = F.init_state(shapes_of(model))['id_embedding.weight'].numpy()
    np.testing.assert_array_equal(eng.encode_items(ids).numpy(), w0[ids.numpy()])
    np.testing.assert_array_equal(eng.table_copy().numpy(), w0)
    with pytest.raises(IndexError):
        eng.encode_items(torch.tensor([61]))


# ------------------------------------------------------------------ two gloo ranks through FlatDDP
def _ddp_worker(rank, port, out_path):
    import torch.distributed as dist
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.optim as O
    for name, f in (('id_index', id_index), ('id_grad_sum', id_grad_sum), ('id_index_ws_ints', id_index_ws_ints)):
        setattr(sim_lib, name, f)
    for mod in (E, EI, O):
        mod.L = sim_lib
    E.TransRecEngine._require_device = lambda self, p0: None
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=2)
    try:
        from adapter4rec_amd.ddp import FlatDDP
        from adapter4rec_amd.optim import FusedAdam
        model, fx, _ = build('sasrec')
        model.train()
        ddp = FlatDDP(model)
        opt = FusedAdam([{'params': list(model.parameters()), 'lr': 1e-3}])
        items = torch.from_numpy(fx['items1']).view(4, -1)[2 * rank:2 * rank + 2].reshape(-1)
        mask = torch.from_numpy(fx['mask1'])[2 * rank:2 * rank + 2]
        opt.zero_grad()
        ddp(items, mask, 'cpu').backward()
        g = model.id_embedding.weight.grad.detach().clone()
        opt.step()
        np.savez(out_path + f'.{rank}.npz', g=g.numpy(), w=model.id_embedding.weight.detach().numpy(),
                 u=model.user_encoder.transformer_encoder.layer_norm.weight.detach().numpy())
    finally:
        dist.destroy_process_group()


def test_id_two_gloo_ranks_lock_step(tmp_path):
    """Each rank takes two of the fixture's four users; the averaged table gradient is the single-process gradient of the whole batch when
    both halves carry the same number of valid positions (mean over positions == mean of the two per-rank means), and the parameters stay
    bit-identical across the ranks."""
    import socket
    import torch.multiprocessing as mp
    fx = fixture('sasrec')
    m = fx['mask1'].reshape(4, -1).sum(1)
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / 'r')
    mp.start_processes(_ddp_worker, args=(port, out), nprocs=2, start_method='spawn')
    r0, r1 = np.load(out + '.0.npz'), np.load(out + '.1.npz')
    np.testing.assert_array_equal(r0['w'], r1['w'])
    np.testing.assert_array_equal(r0['u'], r1['u'])
    np.testing.assert_array_equal(r0['g'], r1['g'])
    # the reference's loss is a mean over the batch's valid positions: two ranks of n0, n1 positions average to (n0 L0 + n1 L1) / (n0 + n1) only
    # when n0 == n1; in general the DDP gradient is 0.5 (g0 + g1) with g_k = (N / (2 n_k)) x (the single-process share of rank k's users)
    n0, n1 = m[:2].sum(), m[2:].sum()
    g_single = _single_grad_weighted(fx, n0, n1)
    g = r0['g']
    np.testing.assert_allclose(g, g_single, atol=1e-5 * np.abs(g_single).max(), rtol=0)


def _single_grad_weighted(fx, n0, n1):
    """The single-process table gradient on the concatenated batch, each half's share re-weighted to what its rank's own mean gives."""
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.engine_id as EI
    import adapter4rec_amd.optim as O
    saved = {mod: mod.L for mod in (E, EI, O)}
    req = E.TransRecEngine._require_device
    for name, f in (('id_index', id_index), ('id_grad_sum', id_grad_sum), ('id_index_ws_ints', id_index_ws_ints)):
        setattr(sim_lib, name, f)
    try:
        for mod in saved:
            mod.L = sim_lib
        E.TransRecEngine._require_device = lambda self, p0: None
        parts = []
        for half in (0, 1):
            model, _, _ = build('sasrec')
            model.train()
            mask = torch.from_numpy(fx['mask1']).clone()
            mask.view(4, -1)[2 * (1 - half):2 * (1 - half) + 2] = 0          # the other rank's positions out of the loss
            model(torch.from_numpy(fx['items1']), mask, 'cpu').backward()
            parts.append(model.id_embedding.weight.grad.numpy().copy())
        return 0.5 * (parts[0] + parts[1])
    finally:
        for mod, l in saved.items():
            mod.L = l
        E.TransRecEngine._require_device = req


# ------------------------------------------------------------------ the image entry point with --item_tower id
ID_FLAGS = ['--item_tower', 'id', '--fine_tune_to', 'all', '--adding_adapter_to', 'None', '--lr', '1e-3', '--label_screen', 'id']


def oracle_hr_id(sd, data, max_seq_len=20):
    """HR@10 of the reference's eval_model (data_utils/metrics.py:82-116) restated on the CPU (oracle/ref_cpu.py), the item embeddings being
    the checkpoint's ID table itself (metrics.py:52-63)."""
    import logging
    from oracle import ref_cpu as R
    from adapter4rec_amd.cv.data_utils import read_behaviors, read_images
    keys, name2id = read_images(os.path.join(data, 'toy', 'images_log.tsv'))
    _, _, _, va, _, hv, _ = read_behaviors(os.path.join(data, 'toy', 'users_log.tsv'), keys, name2id, max_seq_len, 5, logging.getLogger('t'))
    osd = {k: v.float() for k, v in sd.items()}
    _, ranks = R.eval_ranks(osd, osd['id_embedding.weight'], va, hv, dict(R.DEFAULT_CFG, max_seq_len=max_seq_len))
    return R.hit_ndcg(ranks)[0]


def id_two_epochs_resume_and_oracle_hr(tmp_path, monkeypatch, dtype='fp32'):
    """Two epochs, the logged validation HR@10 against the oracle on the saved checkpoint, then a resume from epoch 1 that repeats the
    uninterrupted run's second epoch."""
    import test_cv_run as CR
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    common = ['--root_data_dir', data] + CR.COMMON_CV + ID_FLAGS
    common[common.index('--compute_dtype') + 1] = dtype
    a = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--epoch', '2'], monkeypatch, a)
    assert a['batch'] == [16, 16, 8] * 2, a['batch']
    assert all(np.isfinite(a['loss']))
    ckpts = sorted(os.path.join(dp, f) for dp, _, fs in os.walk('.') for f in fs if f.endswith('.pt'))
    names = [os.path.basename(c) for c in ckpts]
    assert names[0] == 'epoch-1.pt', ckpts
    sd = torch.load(ckpts[-1], map_location='cpu', weights_only=False)['model_state_dict']
    assert 'id_embedding.weight' in sd and not any('cv_encoder' in k for k in sd)
    hr = oracle_hr_id(sd, data)
    valids = [h for m, h in a['eval'] if m == 'valid']
    assert abs(valids[len(names) - 1] - hr) < 1e-3, (valids, hr)
    if len(ckpts) > 1:
        os.remove(ckpts[1])
    b = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--epoch', '1', '--load_ckpt_name', 'epoch-1.pt'], monkeypatch, b)
    assert b['batch'] == [16, 16, 8]
    np.testing.assert_allclose(b['loss'], a['loss'][3:], rtol=2e-3, atol=2e-3)
    c = dict(loss=[], batch=[], eval=[])
    CR._run_cv(common + ['--epoch', '1', '--mode', 'test', '--load_ckpt_name', 'epoch-1.pt'], monkeypatch, c)
    assert [m for m, _ in c['eval']] == ['valid', 'test']
    return a


def test_id_runner_simulated_two_epochs_resume_oracle_hr(simulated, tmp_path, monkeypatch):
    import test_cv_run as CR
    import adapter4rec_amd.engine_id as EI
    CR._simulate_cv(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    id_two_epochs_resume_and_oracle_hr(tmp_path, monkeypatch)


@pytest.mark.parametrize('flags', [['--fine_tune_to', 'None', '--adding_adapter_to', 'None'],
                                   ['--fine_tune_to', 'all', '--adding_adapter_to', 'all']])
def test_id_runner_refuses_other_flag_combinations(flags):
    from adapter4rec_amd.cv import run_adapter as RA
    from adapter4rec_amd.cv.parameters import parse_args
    args = parse_args(['--item_tower', 'id'] + flags)
    with pytest.raises(ValueError, match='--fine_tune_to all and --adding_adapter_to None'):
        RA.train(args, False, 0, None, None, '.', 0.0)
    with pytest.raises(ValueError, match='--item_tower id'):
        RA.test(args, False, 0, None, None, '.', 0.0)
