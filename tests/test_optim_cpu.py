"""CPU: FusedAdam with weight decay, FusedAdamW and gradient-norm clipping -- constructor checks, the host logic on the simulated library (tests/sim_lib.py
plus tests/sim_optim.py) against torch.optim.Adam / AdamW + clip_grad_norm_, checkpoints, the runners' flags, two gloo ranks, and the argument checks of
the new C entry points (they return A4R_EINVAL before any launch, so they run without a GPU)."""
import copy
import ctypes
import glob
import json
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sim_lib
import sim_optim

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def simulated(monkeypatch):
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.optim as O
    monkeypatch.setattr(E, 'L', sim_lib)
    monkeypatch.setattr(O, 'L', sim_lib)
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)
    sim_optim.install(monkeypatch)


# ------------------------------------------------------------------------------------------------------------------ constructor

def test_constructors_accept_weight_decay_and_adamw():
    from adapter4rec_amd.optim import FusedAdam, FusedAdamW
    w = [torch.nn.Parameter(torch.zeros(3))]
    a = FusedAdam(w, weight_decay=0.01)
    assert a.param_groups[0]['weight_decay'] == 0.01 and a.param_groups[0]['decoupled_weight_decay'] is False
    b = FusedAdamW(w)
    assert b.param_groups[0]['weight_decay'] == 0.01 and b.param_groups[0]['decoupled_weight_decay'] is True
    c = FusedAdamW([{'params': w, 'weight_decay': 0.2}], max_grad_norm=1.0)
    assert c.param_groups[0]['weight_decay'] == 0.2 and c.max_grad_norm == 1.0 and c.last_grad_norm is None
    assert FusedAdam(w, decoupled_weight_decay=True, weight_decay=0.1).param_groups[0]['decoupled_weight_decay'] is True
    # torch.optim.Adam's own keys, so that the groups load into torch's optimizers and back
    assert set(torch.optim.AdamW(w).param_groups[0]) <= set(b.param_groups[0])


@pytest.mark.parametrize('kw', [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(foreach=True),
                                dict(fused=True)])
def test_unsupported_arguments_raise(kw):
    from adapter4rec_amd.optim import FusedAdam, FusedAdamW
    w = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (FusedAdam, FusedAdamW):
        with pytest.raises(NotImplementedError):
            cls(w, **kw)
    with pytest.raises(NotImplementedError):
        FusedAdam([{'params': w, **kw}])


def test_bad_values_raise():
    from adapter4rec_amd.optim import FusedAdam, FusedAdamW
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedAdam(w, weight_decay=-0.1)
    with pytest.raises(ValueError):
        FusedAdamW([{'params': w, 'weight_decay': -1.0}])
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            FusedAdamW(w, max_grad_norm=bad)


# ------------------------------------------------------------------------------------------------------------------ host logic vs torch

def _fresh():
    from test_engine_host_logic import build_cpu
    return build_cpu('houlsby')


def _replay(make_opt, ref_cls, ref_kw, max_norm, steps=3):
    """FusedAdam(W) on the simulated engine; torch's optimizer (+ clip_grad_norm_) replayed on clones fed the same gradients."""
    from adapter4rec_amd.inject import optimizer_groups
    root, args, fx, items, mask = _fresh()
    names = [n for n, p in root.named_parameters() if p.requires_grad]
    params = dict(root.named_parameters())
    clones = {n: torch.nn.Parameter(params[n].detach().clone()) for n in names}
    opt = make_opt(optimizer_groups(root, args))
    by_id = {id(p): n for n, p in params.items()}
    ref = ref_cls([{'params': [clones[by_id[id(p)]] for p in g['params']], 'lr': g['lr'], **ref_kw} for g in opt.param_groups])
    norms = []
    for _ in range(steps):
        opt.zero_grad()
        root(items, mask, 'cpu').backward()
        for n in names:
            clones[n].grad = params[n].grad.detach().clone()
        opt.step()
        if max_norm is not None:
            tn = torch.nn.utils.clip_grad_norm_([clones[n] for n in names], max_norm)
            norms.append((float(tn), opt.last_grad_norm))
        ref.step()
        for n in names:
            torch.testing.assert_close(params[n].detach(), clones[n].detach(), rtol=1e-5, atol=1e-7, msg=n)
    return norms


def _norm_step1():
    root, args, fx, items, mask = _fresh()
    root(items, mask, 'cpu').backward()
    return float(torch.nn.utils.get_total_norm([p.grad for p in root.parameters() if p.requires_grad]))


def test_fused_adam_coupled_weight_decay_matches_torch(simulated):
    from adapter4rec_amd.optim import FusedAdam
    _replay(lambda g: FusedAdam(g, weight_decay=0.05), torch.optim.Adam, dict(weight_decay=0.05), None)


def test_fused_adamw_matches_torch(simulated):
    from adapter4rec_amd.optim import FusedAdamW
    _replay(lambda g: FusedAdamW(g, weight_decay=0.05), torch.optim.AdamW, dict(weight_decay=0.05), None)


def test_fused_adamw_clipped_matches_torch(simulated):
    from adapter4rec_amd.optim import FusedAdamW
    m = 0.5 * _norm_step1()
    norms = _replay(lambda g: FusedAdamW(g, weight_decay=0.05, max_grad_norm=m), torch.optim.AdamW, dict(weight_decay=0.05), m)
    assert norms[0][0] > m                                           # the clip is active at step 1
    for want, got in norms:
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - want) <= 1e-6 * want


def test_clipped_step_makes_no_host_read(simulated, monkeypatch):
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdamW
    root, args, fx, items, mask = _fresh()
    opt = FusedAdamW(optimizer_groups(root, args), weight_decay=0.05, max_grad_norm=0.1)
    for s in range(2):                                               # the first step binds the engine; the second runs the bound path
        opt.zero_grad()
        root(items, mask, 'cpu').backward()

        def boom(*a, **k):
            raise AssertionError('host read inside FusedAdamW.step()')
        with monkeypatch.context() as mp_:
            for name in ('item', 'tolist', 'cpu'):
                mp_.setattr(torch.Tensor, name, boom)
            mp_.setattr(torch.cuda, 'synchronize', boom)
            opt.step()
    assert opt.last_grad_norm is not None


def test_flat_gradients_are_not_rewritten(simulated):
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdamW
    root, args, fx, items, mask = _fresh()
    opt = FusedAdamW(optimizer_groups(root, args), max_grad_norm=1e-6)
    opt.zero_grad()
    root(items, mask, 'cpu').backward()
    g = torch.cat([p.grad.reshape(-1) for grp in opt.param_groups for p in grp['params']])
    opt.step()
    assert float(opt.last_grad_norm) > 1e-3
    g = opt._bound.flat_g.clone() if torch.equal(torch.cat([p.grad.reshape(-1) for grp in opt.param_groups for p in grp['params']]), g) else None
    assert g is not None, 'p.grad changed in step()'
    assert torch.equal(opt._bound.flat_g, g) and float(g.norm()) == pytest.approx(float(opt.last_grad_norm), rel=1e-5)


def test_default_path_calls_adam_step_only(simulated, monkeypatch):
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdam, FusedAdamW
    calls = []
    for name in ('adam_step', 'adamw_step', 'grad_sumsq'):
        real = getattr(sim_lib, name)
        monkeypatch.setattr(sim_lib, name, (lambda real, name: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(real, name))
    for make, want in ((lambda g: FusedAdam(g), ['adam_step']), (lambda g: FusedAdamW(g, weight_decay=0.0), ['adam_step']),
                       (lambda g: FusedAdamW(g), ['adamw_step']), (lambda g: FusedAdam(g, max_grad_norm=1.0), ['grad_sumsq', 'adamw_step'])):
        calls.clear()
        root, args, fx, items, mask = _fresh()
        opt = make(optimizer_groups(root, args))
        opt.zero_grad()
        root(items, mask, 'cpu').backward()
        opt.step()
        assert calls == want


def test_state_dict_round_trip_with_torch_adamw(simulated):
    """A FusedAdamW state dict loads into torch.optim.AdamW and back (weight_decay travels in the groups); resuming after 2 steps and taking 1 more
    equals 3 uninterrupted steps bit for bit."""
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdamW

    def run(n, opt, root, items, mask):
        for _ in range(n):
            opt.zero_grad()
            root(items, mask, 'cpu').backward()
            opt.step()

    root, args, fx, items, mask = _fresh()
    groups = optimizer_groups(root, args)
    groups[1]['weight_decay'] = 0.2
    opt = FusedAdamW(groups, weight_decay=0.05, max_grad_norm=0.5)
    run(2, opt, root, items, mask)
    sd_opt = copy.deepcopy(opt.state_dict())
    sd_model = {k: v.clone() for k, v in root.state_dict().items()}
    assert [g['weight_decay'] for g in sd_opt['param_groups']][:2] == [0.05, 0.2]
    ref = torch.optim.AdamW(optimizer_groups(root, args))
    ref.load_state_dict({k: v for k, v in sd_opt.items() if k != 'a4r'})
    assert [g['weight_decay'] for g in ref.param_groups][:2] == [0.05, 0.2] and all(g['decoupled_weight_decay'] for g in ref.param_groups)
    back = copy.deepcopy(ref.state_dict())
    run(1, opt, root, items, mask)
    after3 = {k: v.clone() for k, v in root.state_dict().items()}
    root2, args2, _, _, _ = _fresh()
    root2.load_state_dict(sd_model)
    opt2 = FusedAdamW(optimizer_groups(root2, args2), max_grad_norm=0.5)
    opt2.load_state_dict(back)                                        # torch's AdamW layout, written by torch
    assert [g['weight_decay'] for g in opt2.param_groups][:2] == [0.05, 0.2]
    run(1, opt2, root2, items, mask)
    for k, v in after3.items():
        torch.testing.assert_close(root2.state_dict()[k], v, rtol=0, atol=0)


def test_older_checkpoint_groups_get_defaults(simulated):
    """A state dict of an earlier FusedAdam (groups: lr / betas / eps / weight_decay only) still loads and steps."""
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdam
    root, args, fx, items, mask = _fresh()
    opt = FusedAdam(optimizer_groups(root, args))
    sd = copy.deepcopy(opt.state_dict())
    sd['param_groups'] = [{k: g[k] for k in ('lr', 'betas', 'eps', 'weight_decay', 'params')} for g in sd['param_groups']]
    opt.load_state_dict(sd)
    assert all(g['decoupled_weight_decay'] is False and g['amsgrad'] is False for g in opt.param_groups)
    root(items, mask, 'cpu').backward()
    opt.step()


# ------------------------------------------------------------------------------------------------------------------ entry points

def test_parsers_default_to_the_reference_optimizer():
    from adapter4rec_amd.cv.parameters import parse_args as cv_parse
    from adapter4rec_amd.optim import FusedAdam, FusedAdamW, from_args
    from adapter4rec_amd.parameters import parse_args
    for parse in (parse_args, cv_parse):
        a = parse([])
        assert (a.optimizer, a.weight_decay, a.max_grad_norm) == ('adam', 0.0, 0.0)
        w = [torch.nn.Parameter(torch.zeros(3))]
        opt = from_args([{'params': w, 'lr': 1e-4}], a)
        assert type(opt) is FusedAdam and opt.max_grad_norm is None
        assert opt.param_groups[0]['weight_decay'] == 0 and opt.param_groups[0]['decoupled_weight_decay'] is False
        b = parse(['--optimizer', 'adamw', '--weight_decay', '0.05', '--max_grad_norm', '1'])
        opt = from_args([{'params': w, 'lr': 1e-4}], b)
        assert type(opt) is FusedAdamW and opt.max_grad_norm == 1.0 and opt.param_groups[0]['weight_decay'] == 0.05
        c = parse(['--weight_decay', '0.01'])
        opt = from_args([{'params': w, 'lr': 1e-4}], c)
        assert type(opt) is FusedAdam and opt.param_groups[0]['weight_decay'] == 0.01 and not opt.param_groups[0]['decoupled_weight_decay']


FLAGS = ['--optimizer', 'adamw', '--weight_decay', '0.05', '--max_grad_norm', '1']


def _logged_norms(root):
    lines = [l for f in glob.glob(os.path.join(root, 'work', 'logs_*_train', '*.log')) for l in open(f)]
    return [l for l in lines if 'grad norm:' in l and 'batch loss' in l]


def test_text_runner_adamw_clipped_simulated(tmp_path, monkeypatch):
    import test_text_run as TR
    TR._simulate(monkeypatch)
    sim_optim.install(monkeypatch)
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
              '--adapter_sasrec_lr', '1e-3', '--label_screen', 'adamw', '--mode', 'train', '--epoch', '1']
    rec = dict(loss=[], batch=[], eval=[])
    TR._run(common + FLAGS, monkeypatch, rec)
    assert rec['loss'] and all(x == x for x in rec['loss'])
    assert _logged_norms(root)


def test_cv_id_runner_adamw_clipped_simulated(tmp_path, monkeypatch):
    import test_cv_run as CR
    import test_id_tower_cpu as IC
    import adapter4rec_amd.engine_id as EI
    for n in ('id_index', 'id_grad_sum', 'id_index_ws_ints'):
        if hasattr(IC, n):
            monkeypatch.setattr(sim_lib, n, getattr(IC, n), raising=False)
    CR._simulate_cv(monkeypatch)
    sim_optim.install(monkeypatch)
    monkeypatch.setattr(EI, 'L', sim_lib)
    root = str(tmp_path)
    data = CR._write_tiny(root)
    monkeypatch.chdir(os.path.join(root, 'work'))
    rec = dict(loss=[], batch=[], eval=[])
    CR._run_cv(['--root_data_dir', data] + CR.COMMON_CV + IC.ID_FLAGS + ['--epoch', '1'] + FLAGS, monkeypatch, rec)
    assert rec['loss'] and all(x == x for x in rec['loss'])
    assert _logged_norms(root)


# ------------------------------------------------------------------------------------------------------------------ two ranks

def _ddp_worker(rank, world, port, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import sim_lib as S
    import sim_optim as SO
    import adapter4rec_amd.engine as E
    import adapter4rec_amd.optim as O
    E.L = S
    O.L = S
    S.grad_sumsq, S.adamw_step, S.GRAD_NORM_PARTS = SO.grad_sumsq, SO.adamw_step, SO.GRAD_NORM_PARTS
    E.TransRecEngine._require_device = lambda self, p0: None
    from test_engine_host_logic import build_cpu
    from adapter4rec_amd.ddp import FlatDDP
    from adapter4rec_amd.inject import optimizer_groups
    torch.manual_seed(100 + rank)
    root, args, fx, items, mask = build_cpu('houlsby')
    model = FlatDDP(root)
    opt = O.FusedAdamW(optimizer_groups(model, args), weight_decay=0.05, max_grad_norm=1e-3)
    B = items.shape[0] // 42
    half = B // 2
    my_items = items.view(B, 42, 60)[rank * half:(rank + 1) * half].reshape(-1, 60)
    my_mask = mask[rank * half:(rank + 1) * half]
    norms = []
    for _ in range(2):
        opt.zero_grad()
        model(my_items, my_mask, 'cpu').backward()
        opt.step()
        norms.append(opt.last_grad_norm.clone())
    params = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    torch.save(dict(params=params, norms=norms), os.path.join(out_dir, f'r{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_clip_in_lock_step(tmp_path):
    port = 29000 + (os.getpid() % 500)
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / 'r0.pt'), torch.load(tmp_path / 'r1.pt')
    assert float(r0['norms'][0]) > 1e-3                              # clipping active
    for a, b in zip(r0['norms'], r1['norms']):
        assert torch.equal(a, b)
    for k in r0['params']:
        assert torch.equal(r0['params'][k], r1['params'][k]), k


# ------------------------------------------------------------------------------------------------------------------ bindings and C entry points

def test_binding_validates_before_the_library():
    from adapter4rec_amd import _lib as L
    n = 8
    f = lambda k=n: torch.zeros(k)
    seg_end, seg_group = torch.tensor([n], dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    parts = torch.zeros(L.GRAD_NORM_PARTS, dtype=torch.float64)
    ok = dict(p=f(), g=f(), m=f(), v=f(), seg_end=seg_end, seg_group=seg_group, group_lr=f(1), group_wd=f(1), step=1)
    bad = [dict(g=f(n + 1)), dict(m=torch.zeros(n, dtype=torch.float64)), dict(v=torch.zeros(2 * n)[::2]), dict(seg_end=seg_end.long()),
           dict(seg_group=torch.zeros(2, dtype=torch.int32)), dict(group_wd=f(2)), dict(step=0),
           dict(partials=torch.zeros(10, dtype=torch.float64)), dict(partials=parts, max_norm=0.0), dict(partials=parts, max_norm=float('inf')),
           dict(norm_out=f(1)), dict(partials=parts, max_norm=1.0, norm_out=torch.zeros(1, dtype=torch.float64))]
    for b in bad:
        with pytest.raises(ValueError):
            L.adamw_step(**{**ok, **b})
    with pytest.raises(RuntimeError, match='device tensors'):                 # well-formed host tensors: no CPU fallback
        L.adamw_step(**ok)
    for g, pp in ((torch.zeros(0), parts), (f(), parts.float()), (f(), parts[:10])):
        with pytest.raises(ValueError):
            L.grad_sumsq(g, pp)


def test_c_entries_return_einval_before_launching():
    from adapter4rec_amd import _lib as L
    if torch.cuda.is_available():
        pytest.skip('argument-check probe is a CPU test')
    lib = ctypes.CDLL(L.LIB_PATH)
    P = ctypes.c_void_p
    buf = ctypes.create_string_buffer(1 << 16)                       # host memory: never dereferenced, the checks come first
    x = ctypes.cast(buf, P)
    f = lib.a4r_adamw_step
    f.restype, f.argtypes = L.SIGNATURES['a4r_adamw_step']             # the binding's own declaration (tests/test_abi_cpu.py holds it to the header)
    base = [None, x, x, x, x, 8, x, x, 1, x, 1, 0.9, 0.999, 1e-8, 1.0, x, 1, x, 1.0, x]
    cases = {1: None, 2: None, 3: None, 4: None, 6: None, 7: None, 9: None, 15: None,             # NULL pointers
             5: 0, 8: 0, 10: 0}                                                                  # n <= 0, n_seg <= 0, step < 1
    for i, val in cases.items():
        a = list(base)
        a[i] = val
        assert f(*a) == -1, i
    for dec in (-1, 2):
        a = list(base)
        a[16] = dec
        assert f(*a) == -1, dec
    for mn in (0.0, -1.0, float('nan'), float('inf')):
        a = list(base)
        a[18] = mn
        assert f(*a) == -1, mn
    a = list(base)
    a[17] = None                                                     # norm_out without partials
    assert f(*a) == -1
    s = lib.a4r_grad_sumsq
    s.restype, s.argtypes = L.SIGNATURES['a4r_grad_sumsq']
    assert s(None, None, 8, 1.0, x) == -1 and s(None, x, 8, 1.0, None) == -1 and s(None, x, 0, 1.0, x) == -1 and s(None, x, -3, 1.0, x) == -1
