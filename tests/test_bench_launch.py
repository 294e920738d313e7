"""bench.py's N-rank launch path (the reference starts one process per GPU: Downstream/Text/script/adapter_houlsby.py:58-59,
run.py:685) exercised WITHOUT a GPU: A4R_BENCH_CONTROL_ONLY=1 keeps the self-launch, rendezvous on 127.0.0.1, rank accounting
and the single-JSON-line contract and skips the compute; the backend is gloo.  `--dump-outputs DIR`: its writer on a CPU model, and (GPU)
two bench runs of the same arguments giving the same last-step outputs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, extra_env=None, drop=()):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT') + tuple(drop)}
    env.update(A4R_BENCH_CONTROL_ONLY='1', A4R_BENCH_BACKEND='gloo')
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=600)


def json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith('{')]


def test_self_launch_two_ranks():
    r = run(['--gpus', '2', '--steps', '1', '--warmup', '0'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1, r.stdout                      # ONE line, printed by rank 0
    assert lines[0]['n_gpus'] == 2 and lines[0]['rccl_ranks'] == 2


def test_single_rank_needs_no_launcher():
    r = run(['--gpus', '1'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]['n_gpus'] == 1 and lines[0]['rccl_ranks'] == 1


def test_full_is_accepted_by_the_launch_path():
    """--full (the legs beyond the headline figure) is an option of every run, the self-launched ranks included: it reaches them on their command line."""
    for gpus in ('1', '2'):
        r = run(['--gpus', gpus, '--steps', '1', '--warmup', '0', '--full'])
        assert r.returncode == 0, r.stderr[-2000:]
        lines = json_lines(r.stdout)
        assert len(lines) == 1 and lines[0]['n_gpus'] == int(gpus), r.stdout


def test_rank_count_mismatch_is_an_error():
    """Under a launcher that gives fewer ranks than --gpus the run must fail instead of printing n_gpus of a job that did not run."""
    r = run(['--gpus', '4'], extra_env=dict(WORLD_SIZE='1', RANK='0', LOCAL_RANK='0'))
    assert r.returncode != 0
    assert not json_lines(r.stdout)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location('a4r_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    """--dump-outputs (no GPU: the writer on a CPU model): loss, the trainable parameters' .grad and values in named_parameters() order,
    float32; frozen parameters left out; an array over the cap is a fixed seeded sample, the same positions run after run."""
    import numpy as np
    import torch
    B = _bench_module()
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    model[0].bias.requires_grad = False
    loss = model(torch.randn(5, 3)).square().sum()
    loss.backward()
    rec = B.dump_outputs(str(tmp_path / 'full'), model, loss)
    ps = [p for p in model.parameters() if p.requires_grad]
    want = dict(loss=np.array([loss.item()], np.float32), grads=torch.cat([p.grad.reshape(-1) for p in ps]).numpy(),
                params=torch.cat([p.detach().reshape(-1) for p in ps]).numpy())
    for name, w in want.items():
        got = np.load(tmp_path / 'full' / (name + '.npy'))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, w)
        assert rec['arrays'][name] == dict(elements=w.size, written=w.size, sampled=False, dtype='float32')
    B.DUMP_MAX_ELEMS = 7
    B.dump_outputs(str(tmp_path / 's1'), model, loss)
    B.dump_outputs(str(tmp_path / 's2'), model, loss)
    pos = B.dump_positions(want['grads'].size, 7).numpy()
    assert (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < want['grads'].size        # distinct, sorted, in range
    np.testing.assert_array_equal(pos, B.dump_positions(want['grads'].size, 7).numpy())
    for name in ('grads', 'params'):
        s1, s2 = np.load(tmp_path / 's1' / (name + '.npy')), np.load(tmp_path / 's2' / (name + '.npy'))
        assert s1.shape == (7,)
        np.testing.assert_array_equal(s1, s2)
        np.testing.assert_array_equal(s1, want[name][pos])
    big = B.dump_positions(109041728, 1 << 22)
    assert bool((big[1:] > big[:-1]).all()) and int(big[-1]) < 109041728
    np.testing.assert_array_equal(np.load(tmp_path / 's1' / 'loss.npy'), want['loss'])


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_last_timed_step(tmp_path):
    """bench.py --steps K --dump-outputs DIR on the GPU: K timed steps in the JSON line with ms_per_step, the last timed step's outputs under DIR
    (float32, finite, at most 64 MB), and the same arguments give the same outputs on a second run.  With the flag the last timed step starts from the
    seeded trainable state, so after warm-up and several timed steps the two runs still differ only by the order of one step's fp32 atomic
    accumulation."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    got = []
    for run_i in range(2):
        out = tmp_path / f'run{run_i}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '6', '--warmup', '3', '--batch', '8', '--no-roofline',
                            '--no-cpu-baseline', '--dump-outputs', str(out)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = json_lines(r.stdout)
        assert len(lines) == 1, r.stdout
        d = lines[0]
        assert d['steps'] == 6 and d['warmup'] == 3 and d['ms_per_step'] > 0
        arrays = {}
        for name, meta in d['dump_outputs']['arrays'].items():
            a = np.load(out / (name + '.npy'))
            assert a.dtype == np.float32 and a.size == meta['written'] and np.isfinite(a).all(), name
            arrays[name] = a
        assert set(arrays) == {'loss', 'grads', 'params'}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert float(np.abs(arrays['grads']).max()) > 0
        got.append(arrays)
    a, b = got
    assert abs(float(a['loss'][0]) - float(b['loss'][0])) <= 1e-5 * abs(float(b['loss'][0]))
    np.testing.assert_allclose(a['grads'], b['grads'], rtol=1e-3, atol=1e-4 * float(np.abs(b['grads']).max()))
    # the step's update is Adam's first, lr * sign(grad) (lr <= 1.5e-4 here): where a noise-sized gradient changed sign the parameters are
    # 2 lr apart; such elements must be rare and none may be further apart
    dp = np.abs(a['params'] - b['params'])
    assert float(dp.max()) <= 2 * 1.5e-4 * 1.01 and float(np.mean(dp > 1e-6)) < 1e-3, (float(dp.max()), float(np.mean(dp > 1e-6)))


@pytest.mark.gpu
def test_plain_run_leaves_the_full_legs_out():
    """Without --full a run ends with its timed steps: the headline fields are there, and what only --full measures (roofline pass, CPU-oracle
    baseline, host-enqueue burst) is null in the line instead of being run."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', '--batch', '8'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['unit'] == 'user-sequences/sec' and d['higher_is_better'] is True and d['dtype'] == 'bf16'
    assert abs(d['value'] - 8 / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    assert d['roofline'] is None and d['cpu_baseline'] is None and d['host_enqueue_ms_per_step'] is None and d['allreduce_us'] is None


@pytest.mark.gpu
@pytest.mark.parametrize('dump', [False, True])
def test_bench_host_images_leg(tmp_path, dump):
    """--workload vit_lora --host-images (the pinned-host-memory leg after the timed region) with --full's roofline pass after it, with and
    without --dump-outputs: one JSON line carrying both."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'vit_lora', '--host-images', '--steps', '2', '--warmup', '1', '--full',
           '--no-cpu-baseline']
    if dump:
        cmd += ['--dump-outputs', str(tmp_path / 'dump')]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    d = lines[0]
    assert d['steps'] == 2 and d['ms_per_step'] > 0 and d['loss'] == d['loss']
    assert d['host_images']['ms_per_step_with_h2d'] > 0 and d['roofline'] is not None
    assert ('dump_outputs' in d) == dump
    if dump:
        assert all((tmp_path / 'dump' / (n + '.npy')).exists() for n in ('loss', 'grads', 'params'))
