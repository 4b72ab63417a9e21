"""CPU tests of the HiFi-GAN generator's training surface: the torch restatement's gradients against the genuine reference's
(tests/golden/make_golden_hifigan_grad.py; at max_segments = 8 this fails without the detach of the within-pass conv history, at
6.4e-2), `losses.stft_loss` and `Hifi_GAN.train_stage` against the reference's, and the `use_hip_training` switch's refusals."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import losses
from speech_enhancement_mi_amd.hifigan import Generator, Hifi_GAN

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402
import make_golden_hifigan_grad as mgr  # noqa: E402


@pytest.fixture(scope="module")
def gg():
    return np.load(os.path.join(ROOT, "tests", "golden", "hifigan_grad_golden.npz"))


def tiny(dtype=torch.float32, **change):
    cfg = dict(mh.TINY, **change)
    m = Generator(**cfg).eval().to(dtype)
    m.load_state_dict(mh.state_dict(cfg), strict=True)
    return m


@pytest.mark.parametrize("max_segments", [8, 1])
def test_restatement_gradients_match_the_reference(gg, max_segments):
    m = tiny()
    m.max_segments = max_segments
    mix = torch.from_numpy(mh.mixture())
    names = [n for n, _ in m.named_parameters()]
    worst = 0.0
    for c, (a, b, reset) in enumerate(mgr.CALLS):
        m.zero_grad(set_to_none=True)
        pred, before = m.realtime_process(mix[..., a:b], reset=reset)
        ((pred * torch.from_numpy(gg[f"c{c}_R"]).float()).sum() + (before * torch.from_numpy(gg[f"c{c}_Rb"]).float()).sum()).backward()
        assert rel_rms(pred.detach().numpy(), gg[f"c{c}_pred"]) < 1e-5 and rel_rms(before.detach().numpy(), gg[f"c{c}_before"]) < 1e-5
        for n, g in mgr.grads_of(m, names).items():
            ref = gg[f"c{c}_g_{n}"]
            got = mgr.stored(c, n, g)
            if not np.any(ref):
                assert not np.any(got), n    # deconvlist.3.residual*: unused by the forward
                continue
            e = rel_rms(got, ref)
            worst = max(worst, e)
            assert e < 1e-4, (c, n, e)
    print(f"max_segments {max_segments}: worst gradient rel rms {worst:.2e}")
    for n, p in m.named_parameters():
        assert (p.grad is None) == n.startswith(("deconvlist.3.residual.", "deconvlist.3.residualmask.")), n


def test_stft_loss_and_train_stage_match_the_reference(gg):
    """float64: the loss's |X|^0.3 and |.| amplify a relative forward difference about 4000 times in these gradients, so float32
    (reference and restatement alike) is 1e-4 .. 6e-4 away from float64 (make_golden_hifigan_grad.py); the fixture is the reference
    in float64 and the bound is the 1e-4 of every other gradient test."""
    w = Hifi_GAN([], [], **mh.TINY).eval().double()
    w.generator.load_state_dict(mh.state_dict(mh.TINY), strict=True)
    x, y = torch.from_numpy(mh.mixture()).double()[..., :4800], torch.from_numpy(mgr.target()).double()
    loss = w.train_stage(x, y, stage=2, reset=True)
    loss.backward()
    assert abs(float(loss) - float(gg["ts_loss"][0])) < 1e-4 * abs(float(gg["ts_loss"][0]))
    grads = mgr.grads_of(w.generator, mgr.TS_NAMES)
    for n in mgr.TS_NAMES:
        assert rel_rms(grads[n], gg[f"ts_g_{n}"]) < 1e-4, n
    # the same value from the two outputs handed in: no generator call
    w.generator.reset()
    calls = []
    w.generator.realtime_process = lambda *a, **k: calls.append(a)
    y_hat, y_before = torch.from_numpy(gg["c0_pred"]).double(), torch.from_numpy(gg["c0_before"]).double()
    got = w.train_stage(None, y, stage=2, y_hat=y_hat, y_before=y_before)
    want = 0.5 * losses.stft_loss(y_hat, y, phase=True) + 0.5 * losses.stft_loss(y_before, y, phase=True)
    assert not calls and float(got) == float(want)
    assert abs(float(got) - float(gg["ts_loss"][0])) < 1e-4 * abs(float(gg["ts_loss"][0]))   # c0 is the same call in float32
    assert float(w.train_stage(None, y, stage=1, y_hat=y_hat)) == float(losses.stft_loss(y_hat, y, phase=True))


def test_stft_loss_forms():
    g = torch.Generator().manual_seed(3)
    p, r = torch.randn(2, 1, 1600, generator=g, dtype=torch.float64), torch.randn(2, 1600, generator=g, dtype=torch.float64)
    win = torch.hann_window(200).double()   # the reference builds the window in float32 whatever the signal's dtype
    P, R = (torch.stft(v.reshape(2, 1600), 400, 200, 200, win, return_complex=True) for v in (p, r))
    pm, rm = P.abs().clamp(min=1e-7), R.abs().clamp(min=1e-7)
    plain = (pm.log() - rm.log()).abs().mean() + torch.linalg.norm(pm - rm) / torch.linalg.norm(pm)
    assert abs(float(losses.stft_loss(p, r)) - float(plain)) < 1e-12
    a, b = pm ** 0.3, rm ** 0.3
    ph = 0.7 * (a - b).abs().mean() + 0.3 * torch.view_as_real(a * P / pm - b * R / rm).abs().mean() + torch.linalg.norm(a - b) / torch.linalg.norm(a)
    assert abs(float(losses.stft_loss(p, r, phase=True)) - float(ph)) < 1e-12
    assert float(losses.stft_loss(torch.zeros(1, 800), torch.zeros(1, 800), phase=True)) == 0.0   # the clamp: no NaN at silence


def test_train_stage_refusals():
    w = Hifi_GAN([], [], **mh.TINY).eval()
    x = torch.from_numpy(mh.mixture())[..., :4800]
    y = x[:, 0]
    with pytest.raises(TypeError, match="post=False"):
        w.train_stage(x, y, stage=1)
    with pytest.raises(NotImplementedError, match="discriminators"):
        w.train_stage(x, y, stage=3)
    assert not hasattr(w, "discriminator") and not hasattr(w, "remove_weight_norm")


def test_use_hip_training_switch():
    with pytest.raises(ValueError, match="kernel_size = 5"):
        tiny(kernel_size=5).use_hip_training(True)
    m = tiny(dropout=0.1)
    assert m.hip_training_error() is None      # eval mode: the dropout is inactive
    with pytest.raises(ValueError, match="dropout"):
        m.train().use_hip_training(True)
    assert m._hip_train is False
    assert tiny().hip_training_error() is None and Generator(**mh.FULL).hip_training_error() is None
    m = tiny().use_hip_training(True)
    assert m._hip_train is True and m.use_hip_training(False)._hip_train is False
    m.use_hip_training(True)
    mix = torch.from_numpy(mh.mixture())[..., :3200]
    assert m._choose_path(mix) == "torch"      # a CPU tensor: the restatement, switch or not
    pred, _ = m.realtime_process(mix, reset=True)
    assert m._last_path == "torch" and pred.requires_grad
