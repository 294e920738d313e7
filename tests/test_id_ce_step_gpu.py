"""GPU: one training step and two FusedAdam steps of Model(use_modal=False) with --loss ce against torch autograd on the CPU: the user tower
restated in oracle/ref_cpu.py (the one tests/id_fixture.py pins to the reference's fixtures) with torch's cross_entropy over table[1:] as the
head, on the fixtures' batches and derived initial weights.  Bounds: loss 1e-5 relative, every gradient 1e-5 x max |ref| (check_against_fixture's
rule), parameters after the second Adam step 2e-6 (that file's bound).

Measured on an MI355X (printed by the tests):
    one step, fp32 compute dtype: loss 4.9603348 (reference 4.9603348, relative error 0), worst gradient error 1.19e-06 x max |ref|
    one step, bf16 compute dtype: the same figures (the ID tower's user tower and head run in fp32 under either)
    two FusedAdam steps: worst |parameter - reference| 8.49e-07 (transformer_blocks.0.feed_forward.w_1.weight)
    loss='bce': 1.672733 from the model and from a4r_score_bce_fwd called directly, bit-equal in the recorded runs
"""
import numpy as np
import pytest
import torch

import id_fixture as F
import test_id_tower_cpu as CPU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_REF = {}


def ce_loss(sd, items, mask):
    """The restated model with the cross-entropy head: row (b, t) against every item 1 .. item_num, class = the positive id of position t + 1,
    mean over the rows with log_mask != 0 and a non-pad target."""
    from oracle import ref_cpu as R
    cfg = dict(R.DEFAULT_CFG, arch='sasrec', max_seq_len=F.MAXLEN, embedding_dim=F.E)
    table = sd['id_embedding.weight']
    ids = items.long().view(-1, F.MAXLEN + 1, 2)
    pos_e = table[ids[:, :, 0]]
    prec = R.user_encoder(sd, pos_e[:, :-1], mask, cfg)
    tgt = ids[:, 1:, 0]
    sel = (mask != 0) & (tgt != 0)
    return torch.nn.functional.cross_entropy(prec[sel] @ table[1:].T, tgt[sel] - 1, reduction='mean')


def ce_reference():
    """loss1, every gradient of step 1, every parameter after torch.optim.Adam (lr 1e-3) steps 1 and 2, loss2 -- fp32 on the CPU, computed once."""
    if not _REF:
        model, fx, _ = CPU.build('sasrec', loss='ce')
        params = {k: v.clone().requires_grad_(True) for k, v in F.init_state(CPU.shapes_of(model)).items()}
        opt = torch.optim.Adam(list(params.values()), lr=F.LR)
        for step in (1, 2):
            opt.zero_grad()
            loss = ce_loss(params, torch.from_numpy(fx[f'items{step}']), torch.from_numpy(fx[f'mask{step}']))
            loss.backward()
            params['id_embedding.weight'].grad[0] = 0                 # padding_idx = 0: nn.Embedding never writes row 0's gradient
            _REF[f'loss{step}'] = float(loss.detach())
            if step == 1:
                _REF['grad'] = {k: p.grad.detach().numpy().copy() for k, p in params.items()}
            opt.step()
        _REF['step2'] = {k: p.detach().numpy().copy() for k, p in params.items()}
    return _REF


def build_gpu(dtype, loss='ce'):
    model, fx, _ = CPU.build('sasrec', compute_dtype=dtype, loss=loss)
    return model.to(DEV).train(), fx


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_ce_step_matches_autograd(dtype):
    ref = ce_reference()
    model, fx = build_gpu(dtype)
    loss = model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0)
    loss.backward()
    fig = f'GPU id ce step {dtype}: loss {loss.item():.7f} ref {ref["loss1"]:.7f} rel {abs(loss.item() - ref["loss1"]) / abs(ref["loss1"]):.2e};'
    worst = 0.0
    for k, p in model.named_parameters():
        want = ref['grad'][k]
        worst = max(worst, float(np.abs(p.grad.cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30)))
    print(fig, f'worst gradient error / max |ref| {worst:.2e}')
    assert abs(loss.item() - ref['loss1']) <= 1e-5 * abs(ref['loss1'])
    CPU.check_grads(model, ref)
    g = model.id_embedding.weight.grad.cpu().numpy()
    touched = np.unique(fx['items1'])
    absent = np.setdiff1d(np.arange(1, g.shape[0]), touched)
    assert len(absent) and np.all(np.any(g[absent] != 0, axis=1))          # dense: every item is a candidate of every trained row
    assert np.all(g[0] == 0)


def test_ce_two_fused_adam_steps_match_autograd():
    from adapter4rec_amd.optim import FusedAdam
    ref = ce_reference()
    model, fx = build_gpu('fp32')
    opt = FusedAdam([{'params': list(model.parameters()), 'lr': F.LR}])
    for step, (it, m) in enumerate((('items1', 'mask1'), ('items2', 'mask2')), 1):
        opt.zero_grad()
        loss = model(torch.from_numpy(fx[it]), torch.from_numpy(fx[m]), 0)
        loss.backward()
        opt.step()
        assert abs(loss.item() - ref[f'loss{step}']) <= 1e-5 * abs(ref[f'loss{step}'])
    errs = {k: float(np.abs(p.detach().cpu().numpy() - ref['step2'][k]).max()) for k, p in model.named_parameters()}
    k = max(errs, key=errs.get)
    print(f'GPU id ce two Adam steps: worst |param - ref| {errs[k]:.2e} ({k})')
    w0 = F.init_state(CPU.shapes_of(model))['id_embedding.weight'].numpy()
    assert np.array_equal(model.id_embedding.weight.detach().cpu().numpy()[0].view(np.uint32), w0[0].view(np.uint32))       # the pad row never moves
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref['step2'][k], atol=2e-6, rtol=0, err_msg=k)


def test_ce_device_ids_equal_host_ids():
    """The same batch handed over on the device and on the host.  The cross-entropy head and the ID kernels are deterministic; the user tower's
    weight-gradient flushes use fp32 atomics (existing kernels), so the two steps agree to their summation order: 1e-6 relative."""
    model, fx = build_gpu('bf16')
    a = model(torch.from_numpy(fx['items1']).to(DEV), torch.from_numpy(fx['mask1']).to(DEV), 0)
    a.backward()
    g = model.id_embedding.weight.grad.clone()
    model.zero_grad()
    b = model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0)
    b.backward()
    assert abs(a.item() - b.item()) <= 1e-6 * abs(b.item())
    g2 = model.id_embedding.weight.grad
    assert float((g - g2).abs().max()) <= 1e-6 * float(g2.abs().max())


def test_bce_loss_is_the_bce_head_called_directly():
    """loss='bce' on the same model still runs a4r_score_bce_fwd on the same operands: the head called directly on the step's own embeddings and
    user vectors gives bit-equal scores and count.  Its loss is a sum of fp32 atomics (a4r_head.hip), whose order is not fixed from one launch to
    the next, so the two loss values are compared first bit for bit and, where the order differed, to that order: 1e-6 relative -- the bound of
    test_id_tower_gpu.py::test_id_device_ids_equal_host_ids."""
    from adapter4rec_amd import _lib as L
    model, fx = build_gpu('fp32', loss='bce')
    with torch.no_grad():
        loss = model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0)
    eng = model._engine()
    c = eng._ctx
    assert eng.loss == 'bce' and 'pos' in c and 'lse' not in c
    B, Lq = c['B'], eng.Lseq
    pos, neg, ws = torch.zeros_like(c['pos']), torch.zeros_like(c['neg']), torch.zeros(4, device=DEV)
    L.score_bce_fwd(c['emb'], c['prec'], c['lm'], pos, neg, ws, B, Lq, eng.E, False)
    assert torch.equal(pos.view(torch.int32), c['pos'].view(torch.int32)) and torch.equal(neg.view(torch.int32), c['neg'].view(torch.int32))
    assert float(ws[2]) == float(c['ws'][0, 2])
    same_bits = torch.equal(ws[0].view(torch.int32), loss.view(torch.int32))
    print(f'GPU id bce loss {loss.item():.9f} direct {ws[0].item():.9f} bit-equal {same_bits}')
    assert same_bits or abs(ws[0].item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert abs(loss.item() - float(fx['loss1'])) <= 1e-5 * abs(float(fx['loss1']))
