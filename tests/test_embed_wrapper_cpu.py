"""CPU: the host-side argument checks of _lib.embed_bwd run before any launch, and sim_lib.embed_bwd follows the padding_idx rule
of include/a4r.h (no GPU needed: the checks raise before the wrapper asks for device tensors)."""
import pytest
import torch

from adapter4rec_amd import _lib as L


def args(S=6, H=16, V=20, P=None, roberta=False, pad=0, n_items=3):
    ids = torch.randint(0, V, (n_items, 2 * S))
    P = P if P is not None else (S + pad + 1 if roberta else S)
    return dict(ids=ids, dpre=torch.randn(n_items * S, H), dword=torch.zeros(V, H), dpos=torch.zeros(P, H),
                n_items=n_items, S=S, roberta=roberta, pad_id=pad)


def call(a):
    L.embed_bwd(a['ids'], a['dpre'], a['dword'], a['dpos'], a['n_items'], a['S'], roberta=a['roberta'], pad_id=a['pad_id'])


@pytest.mark.parametrize('roberta', [False, True])
def test_embed_bwd_valid_arguments_reach_the_device_check(roberta):
    a = args(roberta=roberta, pad=int(roberta))
    with pytest.raises(RuntimeError, match='device tensors'):
        call(a)
    a['dword'] = None
    with pytest.raises(RuntimeError, match='device tensors'):
        call(a)


BAD = {
    'ids int32': lambda a: a.update(ids=a['ids'].int()),
    'ids column stride': lambda a: a.update(ids=a['ids'].t().contiguous().t()),
    'ids too narrow': lambda a: a.update(ids=a['ids'][:, :a['S'] - 1]),
    'dpre too short': lambda a: a.update(dpre=a['dpre'][:-1]),
    'dword bf16': lambda a: a.update(dword=a['dword'].bfloat16()),
    'dword width': lambda a: a.update(dword=torch.zeros(20, 17)),
    'dword not contiguous': lambda a: a.update(dword=torch.zeros(16, 20).t()),
    'dpos fp64': lambda a: a.update(dpos=a['dpos'].double()),
    'dpos width': lambda a: a.update(dpos=torch.zeros(a['dpos'].shape[0], 8)),
    'dpos strided rows': lambda a: a.update(dpos=torch.zeros(a['dpos'].shape[0], 32)[:, :16]),
    'dpos too few rows': lambda a: a.update(dpos=a['dpos'][:-1]),
}


@pytest.mark.parametrize('roberta', [False, True])
@pytest.mark.parametrize('what', list(BAD))
def test_embed_bwd_rejects_bad_arguments_on_the_host(what, roberta):
    a = args(roberta=roberta, pad=int(roberta))
    BAD[what](a)
    with pytest.raises(AssertionError):
        call(a)


def test_sim_embed_bwd_padding_rows():
    """The simulated library: word row pad_id and RoBERTa's position row pad_id get nothing; a negative id -(r + 1) adds into row r."""
    import sim_lib as SL
    S, H = 5, 4
    ids = torch.tensor([[3, 1, -6, 1, 2] + [1] * S])
    g = torch.arange(1, S + 1, dtype=torch.float32)[:, None].expand(S, H)
    for roberta, pad in ((False, 0), (True, 1)):
        dword, dpos = torch.zeros(8, H), torch.zeros(S + 2, H)
        raw = ids.clone()
        if not roberta:
            raw[0, :S] = torch.where(raw[0, :S] == 1, torch.zeros_like(raw[0, :S]), raw[0, :S])
        SL.embed_bwd(raw, g, dword, dpos, 1, S, roberta=roberta, pad_id=pad)
        assert torch.equal(dword[pad], torch.zeros(H))
        assert torch.equal(dword[5], torch.full((H,), 3.0)) and torch.equal(dword[3], torch.full((H,), 1.0))
        if roberta:                                       # pids: 2, 1, 1, 1, 3 (the negative id counts as a pad)
            assert torch.equal(dpos[:, 0], torch.tensor([0.0, 0.0, 1.0, 5.0, 0.0, 0.0, 0.0]))
        else:
            assert torch.equal(dpos[:S, 0], torch.arange(1, S + 1, dtype=torch.float32))
