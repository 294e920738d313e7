"""The ID item tower's fixtures (tests/golden/cv_id_{sasrec,cpc}.npz, written by tools/gen_golden_r7.py from the imported reference) and the CPU
restatement the tests compare against.

The fixtures stay small: the initial weights are not stored but derived (init_state: one seeded normal draw per tensor, in state_dict order), and
only what pins the restatement is stored -- the two losses, the gradient of the ID table and of every vector / position table, two fixed random
projections of every matrix gradient, and the table and vectors after the second Adam step.  id_reference_step then recomputes EVERY gradient and
every parameter after two torch.optim.Adam steps through oracle/ref_cpu.py (user tower, scoring head) with autograd; tests check it against the
fixture first (check_against_fixture) and the native paths against its full output."""
import os

import numpy as np
import torch

from golden_util import GOLDEN

ITEM_NUM, E, MAXLEN = 60, 64, 20
LR = 1e-3


def fixture(arch):
    return np.load(os.path.join(GOLDEN, f'cv_id_{arch}.npz'))


def init_state(shapes):
    """{name: shape} in state_dict order -> the fixtures' initial weights: xavier-normal scale for matrices (the ID table's row 0 included),
    1 + 0.1 N for LayerNorm weights, 0.1 N for biases."""
    out = {}
    for i, (k, shape) in enumerate(shapes.items()):
        n = np.random.default_rng([7, i]).standard_normal(shape).astype(np.float32)
        if len(shape) == 2:
            v = n * np.float32(np.sqrt(2.0 / (shape[0] + shape[1])))
        elif k.endswith('layer_norm.weight'):
            v = np.float32(1.0) + np.float32(0.1) * n
        else:
            v = np.float32(0.1) * n
        out[k] = torch.from_numpy(v.astype(np.float32))
    return out


def stored_grad(k, shape):
    """Gradients stored in full: the ID table's, the position table's and every vector's; the rest through their projections."""
    return len(shape) == 1 or 'id_embedding' in k or 'position_embedding' in k


def projections(g):
    """Two fixed random projections of a matrix gradient [r, c]: g @ u [r] and v @ g [c]."""
    r, c = g.shape
    u = np.random.default_rng([11, r, c]).standard_normal(c).astype(np.float64)
    v = np.random.default_rng([13, r, c]).standard_normal(r).astype(np.float64)
    g = np.asarray(g, np.float64)
    return g @ u, v @ g


def _loss(sd, items, mask, arch):
    from oracle import ref_cpu as R
    cfg = dict(R.DEFAULT_CFG, arch=arch, max_seq_len=MAXLEN, embedding_dim=E)
    embs = sd['id_embedding.weight'][items.long()].view(-1, MAXLEN + 1, 2, E)          # model.py:55-58 (nn.Embedding lookup)
    pos_e, neg_e = embs[:, :, 0], embs[:, :, 1]
    prec = R.user_encoder(sd, pos_e[:, :-1], mask, cfg)
    return R.score_loss(prec, pos_e[:, 1:], neg_e[:, :-1], mask, cfg)[0]


def id_reference_step(arch, shapes):
    """The restated reference on the fixture's two batches: loss1, every gradient of step 1, every parameter after torch.optim.Adam
    (lr 1e-3) steps 1 and 2, loss2 -- fp32 on the CPU."""
    fx = fixture(arch)
    params = {k: v.clone().requires_grad_(True) for k, v in init_state(shapes).items()}
    opt = torch.optim.Adam(list(params.values()), lr=LR)
    out = {}
    for step in (1, 2):
        opt.zero_grad()
        loss = _loss(params, torch.from_numpy(fx[f'items{step}']), torch.from_numpy(fx[f'mask{step}']), arch)
        loss.backward()
        params['id_embedding.weight'].grad[0] = 0                     # padding_idx = 0: nn.Embedding never writes row 0's gradient
        out[f'loss{step}'] = float(loss.detach())
        if step == 1:
            out['grad'] = {k: p.grad.detach().numpy().copy() for k, p in params.items()}
        opt.step()
    out['step2'] = {k: p.detach().numpy().copy() for k, p in params.items()}
    return out


def check_against_fixture(ref, fx, tol=1e-5):
    """The restatement reproduces what the imported reference stored (losses, stored gradients, projections, step-2 values)."""
    for s in (1, 2):
        assert abs(ref[f'loss{s}'] - float(fx[f'loss{s}'])) <= 1e-6 * abs(float(fx[f'loss{s}'])), (s, ref[f'loss{s}'], float(fx[f'loss{s}']))
    for k, g in ref['grad'].items():
        if stored_grad(k, g.shape):
            want = fx['grad/' + k]
            np.testing.assert_allclose(g, want, atol=tol * max(np.abs(want).max(), 1e-30), rtol=0, err_msg=k)
        else:
            for j, (a, b) in enumerate(zip(projections(g), (fx['gradproj_u/' + k], fx['gradproj_v/' + k]))):
                np.testing.assert_allclose(a, b, atol=tol * max(np.abs(b).max(), 1e-30), rtol=0, err_msg=f'{k} projection {j}')
        if 'step2/' + k in fx:
            np.testing.assert_allclose(ref['step2'][k], fx['step2/' + k], atol=2e-6, rtol=0, err_msg=k)
