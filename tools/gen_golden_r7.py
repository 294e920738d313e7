#!/usr/bin/env python
"""Generate tests/golden/cv_id_sasrec.npz and cv_id_cpc.npz by IMPORTING the reference's image-path model classes with use_modal=False
(the IDRec baseline: nn.Embedding(item_num + 1, E, padding_idx=0) in front of the SASRec / CPC user tower; CPU, build container only).

Two batches of four users with left-padded short histories (pad slots), an item repeated within a user, across users and as a negative,
and rows touched in step 1 only.  The initial weights are tests/id_fixture.py: init_state (derived, not stored).  Stored: loss of steps 1 and 2
under torch.optim.Adam (lr 1e-3, the reference's Adam(model.parameters(), lr=args.lr)), the step-1 gradients of the ID table, the position table
and every vector in full and two fixed projections of every matrix gradient, and the table and vectors after step 2 (id_fixture.py says why)."""
import argparse
import os
import sys

import numpy as np
import torch

REF = '/root/reference/Downstream/CV'
sys.path.insert(0, REF)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')

from model import Model, ModelCPC  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import id_fixture as F  # noqa: E402

NB = 4
ITEM_NUM, E, MAXLEN = F.ITEM_NUM, F.E, F.MAXLEN
L = MAXLEN + 1


def make_args():
    return argparse.Namespace(max_seq_len=MAXLEN, l2_weight=0, embedding_dim=E, num_attention_heads=2, drop_rate=0.0, transformer_block=2,
                              CV_model_load='vit-base-patch16-224')


def batch(rng, hist_lens, rep_item, only_items):
    """[NB * L * 2] ids (p0 n0 p1 n1 ... per user, left padded with 0 as BuildTrainDataset(use_modal=False) does) + log_mask [NB, L - 1]."""
    ids = np.zeros((NB, L, 2), np.int64)
    mask = np.zeros((NB, L - 1), np.float32)
    for u, n in enumerate(hist_lens):
        seq = rng.choice(only_items, size=n, replace=True)
        if u < 2:
            seq[min(1, n - 1)] = rep_item            # the same item for two users ...
            seq[-1] = rep_item                       # ... and twice within one user
        neg = rng.choice(only_items, size=n, replace=True)
        neg[0] = rep_item                            # ... and as a negative
        ids[u, L - n:, 0] = seq
        ids[u, L - n:, 1] = neg
        mask[u, L - n:L - 1] = 1.0
    return torch.from_numpy(ids.reshape(-1)), torch.from_numpy(mask)


def gen(cls, name):
    model = cls(make_args(), ITEM_NUM, False, None)
    model.load_state_dict(F.init_state({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    rng = np.random.default_rng(3)
    both = np.arange(1, 41)
    items1, mask1 = batch(rng, [21, 6, 13, 3], 5, np.arange(1, 51))          # ids 41..50 only in step 1
    items2, mask2 = batch(rng, [9, 21, 4, 17], 5, both)
    opt = torch.optim.Adam(model.parameters(), lr=F.LR)
    out = {}
    model.train()
    opt.zero_grad()
    loss1 = model(items1, mask1, 'cpu')
    loss1.backward()
    out['loss1'] = loss1.item()
    for k, p in model.named_parameters():
        g = p.grad.detach().numpy().copy()
        if F.stored_grad(k, g.shape):
            out['grad/' + k] = g
        else:
            out['gradproj_u/' + k], out['gradproj_v/' + k] = F.projections(g)
    assert np.all(out['grad/id_embedding.weight'][0] == 0)
    opt.step()
    opt.zero_grad()
    loss2 = model(items2, mask2, 'cpu')
    loss2.backward()
    out['loss2'] = loss2.item()
    opt.step()
    for k, p in model.named_parameters():
        if F.stored_grad(k, tuple(p.shape)):
            out['step2/' + k] = p.detach().numpy().copy()
    out.update(items1=items1.numpy(), mask1=mask1.numpy(), items2=items2.numpy(), mask2=mask2.numpy(), item_num=ITEM_NUM,
               keys=np.array(list(model.state_dict().keys())), params=np.array([k for k, _ in model.named_parameters()]))
    np.savez_compressed(os.path.join(OUT, name), **out)
    print(name, 'loss', out['loss1'], out['loss2'], os.path.getsize(os.path.join(OUT, name)), 'bytes')


if __name__ == '__main__':
    gen(Model, 'cv_id_sasrec.npz')
    gen(ModelCPC, 'cv_id_cpc.npz')
