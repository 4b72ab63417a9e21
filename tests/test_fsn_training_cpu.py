"""FullSubNet training, CPU side: the torch-autograd restatement of realtime_process(train=False) (fsn_training.TrainableFullSubNet,
the checker of the HIP training kernels) against the genuine reference's gradients (tests/golden/fsn_grad_golden.npz,
make_golden_fsn_grad.py): pred and every parameter's gradient of a flag=False chunk and the flag=True chunk that continues it."""
import os

import numpy as np
import pytest
import torch

from conftest import FSN_TINY, ROOT, fsn_spec, rel_rms

CHUNKS = ((0, 4800, False), (4800, 8000, True))


@pytest.fixture(scope="module")
def ggolden():
    return np.load(os.path.join(ROOT, "tests", "golden", "fsn_grad_golden.npz"))


def _tiny_model():
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    m = TrainableFullSubNet(**FSN_TINY)
    sd = synth.make_state_dict(fsn_spec(FSN_TINY), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def test_restatement_vs_reference_gradients(ggolden):
    from speech_enhancement_mi_amd import synth
    m = _tiny_model().double()
    mix, clean = synth.synth_utterances(2, 8000, 3, seed=7)
    src = np.repeat(clean[:, None, :], 3, axis=1)
    for c, (a, b, flag) in enumerate(CHUNKS):
        m.zero_grad(set_to_none=True)
        pred, crm, s, x = m.realtime_process(torch.from_numpy(mix[..., a:b]).double(), torch.from_numpy(src[..., a:b]).double(), flag=flag, train=False)
        assert pred.requires_grad and not crm.requires_grad and not s.requires_grad and not x.requires_grad
        assert crm.shape[1:] == (2, 2, 201, 21) and s.shape == crm.shape and x.shape == crm.shape
        assert rel_rms(pred.detach().numpy(), ggolden[f"c{c}_pred"]) <= 1e-5
        (pred * torch.from_numpy(ggolden[f"c{c}_R"]).double()).sum().backward()
        for k, p in m.named_parameters():
            ref = ggolden[f"c{c}_grad.{k}"]
            assert p.grad is not None and np.abs(ref).max() > 0, k
            e = rel_rms(p.grad.numpy(), ref)
            assert e <= 1e-4, f"chunk {c} {k}: rel rms {e:.2e}"


def test_restatement_needs_a_first_chunk():
    from speech_enhancement_mi_amd import synth
    m = _tiny_model()
    mix, _ = synth.synth_utterances(1, 3200, 3, seed=1)
    with pytest.raises(RuntimeError, match="flag=False"):
        m.realtime_process(torch.from_numpy(mix), flag=True, train=False)


def test_state_dict_and_loss_are_fullsubnets():
    from speech_enhancement_mi_amd.fullsubnet import FullSubNet
    m = _tiny_model()
    assert list(m.state_dict()) == list(FullSubNet(**FSN_TINY).state_dict())
    assert m.compute_loss.__func__ is FullSubNet.compute_loss
