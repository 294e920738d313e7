"""GPU: the image entry point with --item_tower id --device_sampler 1 on the real library in bf16 -- the scenario of
tests/test_id_sample_cpu.py (two epochs in batches of [16, 16, 8] with no DataLoader, the logged HR@10 against the CPU oracle on the
checkpoint, a resume that repeats the second epoch batch for batch) for both heads.  --loss ce reads no negative: none may be drawn."""
import pytest

import test_id_sample_cpu as CPU

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('loss', ['bce', 'ce'])
def test_runner_two_epochs_resume_oracle_hr(loss, tmp_path, monkeypatch):
    batches = CPU.sampler_two_epochs_resume_and_oracle_hr(tmp_path, monkeypatch, dtype='bf16', loss=loss)
    if loss == 'ce':
        assert all(not b[:, 1].any() for b in batches)                # the negatives column the engine received
    else:
        assert all((b[:, 1] != 0).any() for b in batches)
    assert all((b[:, 0] != 0).any() for b in batches)
