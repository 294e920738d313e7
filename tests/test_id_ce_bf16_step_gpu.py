"""GPU: one training step of Model(use_modal=False) with --loss ce --ce_dtype bf16 against torch autograd on the CPU: the restated model of
test_id_ce_step_gpu.py::ce_loss with straight-through bf16 rounding of the head's two operands (x + (bf16(x) - x).detach() on prec and on the
table: the head sees the rounded values, the gradients go to the fp32 masters unchanged).

Bounds.  Loss 1e-4 relative: the GPU's fp32 prec differs from the CPU's by about 1e-6, which flips the bf16 rounding of a few elements, and one
flip moves one score by at most 2^-8 |x| |y|.  Gradients, per tensor: max |GPU - ref| / max |ref| is held to four times the value of the first
clean run (MEASURED below; the margin covers the run-to-run atomics of the user tower and rounding flips) and in no case to more than 2^-7, one
bf16 ulp -- above that the error is not rounding.

Measured on an MI355X (printed by the test):
    loss 4.9600344 ref 4.9600339 rel 9.61e-08
    gradients, max |GPU - ref| / max |ref| (the names below user_encoder.transformer_encoder. shortened):
        position_embedding.weight 5.16e-04, layer_norm.weight 3.11e-04, layer_norm.bias 2.29e-04
        transformer_blocks.0.multi_head_attention.w_Q.weight 4.15e-04, transformer_blocks.0.multi_head_attention.w_K.weight 5.44e-04, transformer_blocks.0.multi_head_attention.w_V.weight 3.97e-04
        transformer_blocks.0.multi_head_attention.fc.weight 3.52e-04, transformer_blocks.0.multi_head_attention.layer_norm.weight 4.77e-04, transformer_blocks.0.multi_head_attention.layer_norm.bias 2.63e-04
        transformer_blocks.0.feed_forward.w_1.weight 3.94e-04, transformer_blocks.0.feed_forward.w_1.bias 2.82e-04, transformer_blocks.0.feed_forward.w_2.weight 3.56e-04
        transformer_blocks.0.feed_forward.w_2.bias 2.45e-04, transformer_blocks.0.feed_forward.layer_norm.weight 2.79e-04, transformer_blocks.0.feed_forward.layer_norm.bias 2.95e-04
        transformer_blocks.1.multi_head_attention.w_Q.weight 4.85e-04, transformer_blocks.1.multi_head_attention.w_K.weight 3.64e-04, transformer_blocks.1.multi_head_attention.w_V.weight 2.87e-04
        transformer_blocks.1.multi_head_attention.fc.weight 2.72e-04, transformer_blocks.1.multi_head_attention.layer_norm.weight 7.12e-04, transformer_blocks.1.multi_head_attention.layer_norm.bias 2.20e-04
        transformer_blocks.1.feed_forward.w_1.weight 4.89e-04, transformer_blocks.1.feed_forward.w_1.bias 4.00e-04, transformer_blocks.1.feed_forward.w_2.weight 2.74e-04
        transformer_blocks.1.feed_forward.w_2.bias 2.68e-04, transformer_blocks.1.feed_forward.layer_norm.weight 3.66e-04, transformer_blocks.1.feed_forward.layer_norm.bias 3.10e-04
        id_embedding.weight 6.71e-04
    loss 4.960334778 without the flag 4.960334778 bit-equal True
"""
import numpy as np
import pytest
import torch

import id_fixture as F
import test_id_ce_step_gpu as CE32
import test_id_tower_cpu as CPU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ULP = 2.0 ** -7
MEASURED = {            # parameter name -> max |GPU - ref| / max |ref| of the first clean run (a name that is absent is held to one bf16 ulp alone)
    'user_encoder.transformer_encoder.position_embedding.weight': 5.16e-04,
    'user_encoder.transformer_encoder.layer_norm.weight': 3.11e-04,
    'user_encoder.transformer_encoder.layer_norm.bias': 2.29e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.w_Q.weight': 4.15e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.w_K.weight': 5.44e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.w_V.weight': 3.97e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.fc.weight': 3.52e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.layer_norm.weight': 4.77e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.multi_head_attention.layer_norm.bias': 2.63e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.w_1.weight': 3.94e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.w_1.bias': 2.82e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.w_2.weight': 3.56e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.w_2.bias': 2.45e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.layer_norm.weight': 2.79e-04,
    'user_encoder.transformer_encoder.transformer_blocks.0.feed_forward.layer_norm.bias': 2.95e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.w_Q.weight': 4.85e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.w_K.weight': 3.64e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.w_V.weight': 2.87e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.fc.weight': 2.72e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.layer_norm.weight': 7.12e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.multi_head_attention.layer_norm.bias': 2.20e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.w_1.weight': 4.89e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.w_1.bias': 4.00e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.w_2.weight': 2.74e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.w_2.bias': 2.68e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.layer_norm.weight': 3.66e-04,
    'user_encoder.transformer_encoder.transformer_blocks.1.feed_forward.layer_norm.bias': 3.10e-04,
    'id_embedding.weight': 6.71e-04,
}
_REF = {}


def st_bf16(x):
    return x + (x.bfloat16().float() - x).detach()


def ce_loss_bf16(sd, items, mask):
    """test_id_ce_step_gpu.ce_loss with the head's operands rounded straight-through."""
    from oracle import ref_cpu as R
    cfg = dict(R.DEFAULT_CFG, arch='sasrec', max_seq_len=F.MAXLEN, embedding_dim=F.E)
    table = sd['id_embedding.weight']
    ids = items.long().view(-1, F.MAXLEN + 1, 2)
    prec = R.user_encoder(sd, table[ids[:, :, 0]][:, :-1], mask, cfg)
    tgt = ids[:, 1:, 0]
    sel = (mask != 0) & (tgt != 0)
    return torch.nn.functional.cross_entropy(st_bf16(prec[sel]) @ st_bf16(table)[1:].T, tgt[sel] - 1, reduction='mean')


def reference():
    if not _REF:
        model, fx, _ = CPU.build('sasrec', loss='ce', ce_dtype='bf16')
        params = {k: v.clone().requires_grad_(True) for k, v in F.init_state(CPU.shapes_of(model)).items()}
        items, mask = torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1'])
        loss = ce_loss_bf16(params, items, mask)
        loss.backward()
        params['id_embedding.weight'].grad[0] = 0                     # padding_idx = 0
        _REF['loss1'] = float(loss.detach())
        _REF['grad'] = {k: p.grad.detach().numpy().copy() for k, p in params.items()}
        # the restatement without the rounding is the fp32 test's own reference: the helper above changes the head and nothing else
        plain = CE32.ce_loss({k: v.detach() for k, v in params.items()}, items, mask)
        assert abs(float(plain) - CE32.ce_reference()['loss1']) <= 1e-7 * abs(float(plain))
    return _REF


def test_ce_bf16_step_matches_autograd_with_straight_through_rounding():
    ref = reference()
    model, fx, _ = CPU.build('sasrec', compute_dtype='fp32', loss='ce', ce_dtype='bf16')
    model = model.to(DEV).train()
    loss = model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0)
    eng = model._engine()
    assert eng.ce_dtype == 'bf16' and eng._ctx['ce_cast'] is not None and eng._ctx['ce_cast'][1].dtype == torch.bfloat16
    loss.backward()
    rel = abs(loss.item() - ref['loss1']) / abs(ref['loss1'])
    print(f'GPU id ce bf16 step: loss {loss.item():.7f} ref {ref["loss1"]:.7f} rel {rel:.2e}')
    errs = {}
    for k, p in model.named_parameters():
        want = ref['grad'][k]
        errs[k] = float(np.abs(p.grad.cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30))
    print('GPU id ce bf16 step gradients, max |GPU - ref| / max |ref|: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert rel <= 1e-4
    for k, v in errs.items():
        assert v <= min(4 * MEASURED.get(k, ULP), ULP), (k, v)
    g = model.id_embedding.weight.grad.cpu().numpy()
    absent = np.setdiff1d(np.arange(1, g.shape[0]), np.unique(fx['items1']))
    assert len(absent) and np.all(np.any(g[absent] != 0, axis=1))          # dense: every item is a candidate of every trained row
    assert np.all(g[0] == 0)
    # the rounding is there: the fp32 head's loss on the same weights is another number
    assert abs(ref['loss1'] - CE32.ce_reference()['loss1']) > 1e-7 * abs(ref['loss1'])


def test_ce_dtype_fp32_is_the_fp32_head():
    """ce_dtype='fp32' runs what a model built without the flag runs: no cast, the same loss (the forward holds no atomics: bit for bit in the
    recorded run; 1e-6 relative is what test_id_ce_step_gpu.py allows between two runs), and the fp32 test's reference within its 1e-5."""
    losses = []
    for kw in (dict(ce_dtype='fp32'), dict()):
        model, fx, _ = CPU.build('sasrec', compute_dtype='fp32', loss='ce', **kw)
        model = model.to(DEV).train()
        with torch.no_grad():
            losses.append(model(torch.from_numpy(fx['items1']), torch.from_numpy(fx['mask1']), 0))
        assert model._engine().ce_dtype == 'fp32' and model._engine()._ctx['ce_cast'] is None
    a, b = losses
    print(f'GPU id ce fp32 flag: loss {a.item():.9f} without the flag {b.item():.9f} bit-equal {torch.equal(a.view(torch.int32), b.view(torch.int32))}')
    assert abs(a.item() - b.item()) <= 1e-6 * abs(b.item())
    want = CE32.ce_reference()['loss1']
    assert abs(a.item() - want) <= 1e-5 * abs(want)
