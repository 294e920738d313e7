"""CPU: the engines' block records (adapter4rec_amd/engine_blocks.py) carry declared fields only, whichever of the three builders made them:
the BERT layer loop, the plain-block builder (SASRec and zero-padded K-Adapter blocks) and the ViT layer loop."""
import pytest

import test_engine_cv as TC
import test_engine_host_logic as TH
from adapter4rec_amd.engine_blocks import _Block, _KAdapter

simulated = TC.simulated          # patches engine.py and engine_vit.py (a superset of test_engine_host_logic's fixture)


def _text_engine():
    root, *_ = TH.build_cpu('kadapter')         # the smallest text model, with K-Adapters on both towers
    return getattr(root, 'model', root)._engine()


def _vit_engine():
    root, *_ = TC.build('cv_vit_kadapter')      # the smallest ViT model, with K-Adapters over its token rows and on the user tower
    return getattr(root, 'model', root)._engine()


@pytest.mark.parametrize('build, vit', [(_text_engine, False), (_vit_engine, True)], ids=['text', 'vit'])
def test_every_block_is_a_declared_record(simulated, build, vit):
    eng = build()
    kads = eng.bert_kads + eng.sas_kads
    assert eng.bert_blocks and eng.sas_blocks and eng.bert_kads and eng.sas_kads
    assert all(type(k) is _KAdapter and k.blocks for k in kads)
    groups = [(eng.bert_blocks, vit), (eng.sas_blocks, False)] + [(k.blocks, False) for k in kads]
    for blocks, pre_ln in groups:
        for b in blocks:
            assert type(b) is _Block
            with pytest.raises(AttributeError):
                b.wi_8 = None                       # a misspelt field must not be born silently
            assert b.Hv <= b.H and b.H % 64 == 0
            assert b.wo is b.d_o.w and b.wi is b.d_i.w and b.wo2 is b.d_o2.w
            assert (b.lnA is None) == (not pre_ln)
            assert (b.ln1 is None) == pre_ln
    assert any(b.Hv < b.H for k in eng.sas_kads for b in k.blocks)        # the zero-padded kind is among them (16 wide, stored as 64)
    with pytest.raises(AttributeError):
        kads[0].block = None
