"""De-risking the first multi-rank hardware run on a ONE-GPU box (VERDICT r3 task 6; the reference: Downstream/Text/run.py:503,599,685).

(a) two ranks sharing cuda:0, gloo on DEVICE tensors, the full public path (FlatDDP -> model() -> backward -> FusedAdam) through the real
    HIP library: replicas bit-identical after three steps, the averaged gradients of step 1 equal the IMPORTED reference's under 2-rank
    torch DDP (tests/golden/ddp2_houlsby.npz), per-rank losses equal the reference's.
(b) one rank, backend 'nccl' (= RCCL), A4R_DDP_FORCE=1: the chunked, overlapped exchange (ReduceOp.AVG on views of the flat gradient
    buffer, async on RCCL's stream) leaves the flat buffer equal to the single all-reduce's (to the kernels' atomic-order noise), on the device -- the RCCL calls of
    adapter4rec_amd/ddp.py execute on hardware even where only one GPU is leased.
What neither covers is xGMI itself: more than one DEVICE under RCCL runs only in the driver's SCALE tier.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu


def _paths():
    for p in (HERE, os.path.dirname(HERE)):
        if p not in sys.path:
            sys.path.insert(0, p)


def _two_rank_worker(rank, world, port, out_dir):
    _paths()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)                                        # both ranks on the one GPU (gloo; RCCL refuses duplicate devices)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from test_engine_host_logic import build_cpu
    from adapter4rec_amd.ddp import FlatDDP
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdam
    root, args, fx, items, mask = build_cpu('houlsby')
    with torch.no_grad():                                           # ranks start from DIFFERENT adapter values: the wrapper broadcasts rank 0's
        for p in root.parameters():
            if p.requires_grad:
                p.add_(0.01 * rank)
    root.to('cuda:0').eval()
    model = FlatDDP(root, device_ids=[0], output_device=0)
    opt = FusedAdam(optimizer_groups(model, args))
    B = items.shape[0] // 42
    half = B // 2
    my_items = items.view(B, 42, 60)[rank * half:(rank + 1) * half].reshape(-1, 60).to('cuda:0')
    my_mask = mask[rank * half:(rank + 1) * half].to('cuda:0')
    losses, grads1 = [], None
    for s in range(3):
        opt.zero_grad()
        loss = model(my_items, my_mask, 0)
        loss.backward()
        if s == 0:
            grads1 = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}
        opt.step()
        losses.append(float(loss.detach()))
    params = {n: p.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}
    assert all(p.is_cuda for p in model.parameters())
    torch.save(dict(losses=losses, grads=grads1, params=params), os.path.join(out_dir, f'g{rank}.pt'))
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_device_tensors_vs_reference_ddp(tmp_path):
    port = 29500 + ((os.getpid() + 101) % 500)
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / 'g0.pt'), torch.load(tmp_path / 'g1.pt')
    for k in r0['grads']:
        assert torch.equal(r0['grads'][k], r1['grads'][k]), k        # identical averaged gradients ...
        assert torch.equal(r0['params'][k], r1['params'][k]), k      # ... and replicas in lock-step after 3 Adam steps
    ref = np.load(os.path.join(HERE, 'golden', 'ddp2_houlsby.npz'))  # the imported reference under 2-rank torch DDP, same 2 + 2 user split
    np.testing.assert_allclose([r0['losses'][0], r1['losses'][0]], ref['rank_losses'], atol=1e-4, rtol=0)
    keys = [k for k in ref.files if k.startswith('grad/')]
    assert len(keys) == len(r0['grads'])
    for k in keys:
        want = ref[k]
        np.testing.assert_allclose(r0['grads']['module.' + k[5:]].numpy(), want, atol=1e-6 + 1e-4 * np.abs(want).max(), rtol=0, err_msg=k)
    assert r0['losses'][2] < r0['losses'][0] and r1['losses'][2] < r1['losses'][0]          # both shards improve under the shared update


def _rccl_one_rank_worker(rank, world, port, out_dir):
    _paths()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', A4R_DDP_FORCE='1',
                      HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', '0'))
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)       # RCCL, one rank
    import adapter4rec_amd.engine as E
    from test_engine_shapes import make
    from adapter4rec_amd.ddp import FlatDDP
    from adapter4rec_amd.inject import optimizer_groups
    from adapter4rec_amd.optim import FusedAdam
    model, args, _, ids, mask = make('four_users_wide_adapters', 'cuda:0')
    args.fine_tune_lr, args.lr, args.adapter_bert_lr, args.adapter_sasrec_lr = 5e-5, 1e-4, 1.5e-4, 1.5e-4
    ids, mask = ids.to(dev), mask.to(dev)
    model = FlatDDP(model, device_ids=[0], output_device=0)
    inner = getattr(model.module, 'model', model.module)
    assert inner._a4r_ddp is model and model._avg                 # the exchange is ON with one rank, and it is RCCL's AVG
    opt = FusedAdam(optimizer_groups(model, args))
    opt.zero_grad()
    model(ids, mask, 0).backward()
    opt.step()
    out = {}
    for mode in (True, False):
        E.TransRecEngine.OVERLAP_ALLREDUCE = mode
        if inner._native[0] is not None:
            inner._engine()._chunks = 0
        launches = []
        real = FlatDDP.launch_
        FlatDDP.launch_ = lambda self, flat, lo, hi: (launches.append((lo, hi)), real(self, flat, lo, hi))[1]
        try:
            opt.zero_grad()
            loss = model(ids, mask, 0)
            loss.backward()
        finally:
            FlatDDP.launch_ = real
        torch.cuda.synchronize()
        eng = inner._engine()
        assert eng.flat_g.is_cuda
        out[mode] = dict(flat=eng.flat_g.detach().cpu().clone(), launches=launches, loss=float(loss.detach()))
    # the collective itself: AVG over one rank is the identity, async works joined, on the device
    t = torch.arange(1000, device=dev, dtype=torch.float32)
    model.launch_(t, 100, 900)
    model.wait_all()
    out['identity'] = bool(torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float32)))
    out['any_rank'] = (model.any_rank(torch.tensor(True, device=dev)), model.any_rank(False))
    torch.save(out, os.path.join(out_dir, 'rccl1.pt'))
    dist.destroy_process_group()


def test_one_rank_rccl_chunked_exchange_equals_single_allreduce(tmp_path):
    port = 29500 + ((os.getpid() + 211) % 500)
    mp.spawn(_rccl_one_rank_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / 'rccl1.pt', weights_only=False)
    assert len(r[True]['launches']) >= 2 and len(r[False]['launches']) <= 1, (r[True]['launches'], r[False]['launches'])
    covered = sorted(r[True]['launches'])
    assert all(a[1] <= b[0] for a, b in zip(covered, covered[1:]))                     # disjoint: no element is averaged twice
    # two passes of the same step: identical up to the order of the kernels' fp32 atomic accumulation (the loss sum itself, column sums,
    # embedding rows); a chunk that was dropped, doubled or left in flight would show at O(1)
    assert abs(r[True]['loss'] - r[False]['loss']) <= 1e-5 * abs(r[False]['loss'])
    torch.testing.assert_close(r[True]['flat'], r[False]['flat'], rtol=1e-3, atol=1e-4 * float(r[False]['flat'].abs().max()))
    assert float(r[True]['flat'].abs().max()) > 0
    assert r['identity'] and r['any_rank'] == (True, False)


def test_bench_two_ranks_oversubscribed_json_line():
    """bench.py --gpus 2 end to end on the one GPU (A4R_BENCH_OVERSUBSCRIBE=1: both ranks on cuda:0, gloo -- RCCL refuses duplicate devices):
    self-launch, rendezvous on 127.0.0.1, the flat-gradient exchange on device tensors inside the timed public path, ONE JSON line from rank 0
    with the multi-rank fields the first SCALE record will be read by (VERDICT r3 task 6c); --full for the all-reduce timed on its own."""
    import json
    import subprocess
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(A4R_BENCH_OVERSUBSCRIBE='1', A4R_BENCH_BACKEND='gloo')
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '2', '--batch', '8', '--full', '--no-roofline'],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d['n_gpus'] == 2 and d['rccl_ranks'] == 2 and d['config']['parallelism'] == 'dp2' and d['config']['global_batch'] == 16
    assert len(d['ms_per_step_ranks']) == 2 and d['ms_per_step_spread'] >= 0 and abs(max(d['ms_per_step_ranks']) - d['ms_per_step']) < 0.5
    assert d['allreduce_bytes_per_step'] > 9e6 and d['allreduce_us'] > 0 and d['allreduce_overlapped'] is True
    assert d['value'] > 0 and d['loss'] == d['loss']
