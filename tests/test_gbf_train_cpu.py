"""CPU checks of GeneralBeamformer training: the torch restatement (the checker of the HIP training kernels) against the genuine
reference's gradient fixture, the opt-in switch, and the refusals of use_hip_training."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_gbf as mgb  # noqa: E402


def tiny(**over):
    cfg = dict(mgb.TINY, **over)
    m = GeneralBeamformer(**cfg).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(mgb.spec_of(cfg), seed=0).items()}, strict=True)
    return m


def test_restatement_gradients_match_reference_fixture():
    gg = np.load(os.path.join(ROOT, "tests", "golden", "gbf_grad_golden.npz"))
    m = tiny()
    mix = mgb.mixture()
    for c, (a, b, flag) in enumerate(mgb.CHUNKS):
        m.zero_grad(set_to_none=True)
        pred = m.realtime_process(torch.from_numpy(mix[..., a:b].copy()), torch.tensor([flag, flag]))
        assert m._last_path == "torch"
        assert rel_rms(pred.detach().numpy(), gg[f"c{c}_pred"]) <= 1e-4, c
        (pred * torch.from_numpy(gg[f"c{c}_R"])).sum().backward()
        for k, p in m.named_parameters():
            want = gg[f"c{c}_grad.{k}"]
            got = np.zeros(p.shape, np.float32) if p.grad is None else p.grad.numpy()
            if not np.any(want):   # the last decoder block's unused residual* modules
                assert not np.any(got), (c, k)
                continue
            assert rel_rms(got, want) <= 1e-4, (c, k, rel_rms(got, want))


def test_hip_training_is_opt_in_and_cpu_calls_take_the_restatement():
    m = tiny()
    assert m._hip_train is False
    x = torch.from_numpy(synth.synth_utterances(2, 3200, 3, seed=3)[0])
    y = m.realtime_process(x)
    assert m._last_path == "torch" and y.requires_grad
    assert m.use_hip_training() is m and m._hip_train is True
    y = m.realtime_process(x, torch.tensor([False, False]))   # grad enabled, but a CPU tensor: still the restatement
    assert m._last_path == "torch" and y.requires_grad
    assert m.use_hip_training(False)._hip_train is False


def test_float64_restatement_runs():
    m = tiny().double()
    x = torch.from_numpy(synth.synth_utterances(1, 3200, 3, seed=5)[0]).double()
    y = m.realtime_process(x)
    assert y.dtype == torch.float64 and torch.isfinite(y).all()


def test_use_hip_training_refuses_unsupported_geometry():
    with pytest.raises(ValueError, match="kernel_size = 5"):
        GeneralBeamformer(**dict(mgb.TINY, kernel_size=5)).use_hip_training()
    with pytest.raises(ValueError, match="num_inputs = 2"):
        GeneralBeamformer(**dict(mgb.TINY, num_inputs=2)).use_hip_training()


def test_use_hip_training_refuses_active_dropout():
    m = GeneralBeamformer(**dict(mgb.TINY, dropout=0.1)).train()
    with pytest.raises(ValueError, match="dropout"):
        m.use_hip_training()
    m.eval().use_hip_training()   # dropout is inactive in eval mode
    assert m.hip_training_error() is None
    m.train()
    assert "dropout" in m.hip_training_error()
