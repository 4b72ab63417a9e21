"""GPU tests of the GeneralBeamformer kernel path (general_beamformer.py, csrc/se_gbf.hip): the three head kernels against the torch
restatement's stages in float64, the whole path against the genuine reference's fixture and against the restatement, continuation,
chunking, reproducibility and a 64-utterance batch."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer, _gln
from speech_enhancement_mi_amd.train_net import _p

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_gbf as mgb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F, T, M = 201, 21, 3


def make_model(tag, device=DEV):
    cfg = dict(mgb.GEOMS)[tag]
    m = GeneralBeamformer(**cfg).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(mgb.spec_of(cfg), seed=0).items()}, strict=True)
    return m.to(device)


def kernel_spectrum(m):
    """The restatement's spectrum() on the kernels' STFT, so both sides see the same spectrum (the phase feature jumps by pi where
    re changes sign: DESIGN.md 6 (i))."""
    from speech_enhancement_mi_amd.train_net import _sig

    def spectrum(seg):
        B, Mm, N, Ks = seg.shape
        sig = _sig(seg.device, m._cfg["n_fft"], m._win, m._hop, Ks)
        out = torch.empty(1, B * Mm * N, T, F, 2, device=seg.device)
        K._chk(K._lib().se_sig_stft(sig, _p(seg.contiguous().float()), B * Mm * N, 1, Ks, 0, 0, 1, _p(out), K._st()))
        return out.reshape(B, Mm, N, T, F, 2).permute(0, 1, 2, 4, 3, 5)
    return spectrum


def rng_t(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)).to(DEV)


# ---- the three head kernels against the restatement in float64 ----------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
@torch.no_grad()
def test_psd_kernel(zero):
    m = make_model("tiny")
    B, Nc = 2, 2
    S = B * Nc
    xl = torch.zeros(S, 108, T, F, device=DEV) if zero else rng_t(1, S, 108, T, F)
    spec = rng_t(2, S, M, T, F, 2, scale=3.0)
    for ln, seed in ((m.ln_S, 3), (m.ln_N, 4)):
        ln.weight.data.copy_(rng_t(seed, *ln.weight.shape))
    rows = [torch.full((B * F * Nc * T, 16), float("nan"), device=DEV) for _ in range(2)]
    K._chk(K._lib().se_gbf_psd_fwd(_p(xl), _p(spec), _p(m.ln_S.weight), _p(m.ln_S.bias), _p(m.ln_N.weight), _p(m.ln_N.bias), _p(rows[0]),
                                    _p(rows[1]), S, B, M, T, F, K._st()))
    md = make_model("tiny", "cpu").double()
    md.load_state_dict({k: v.double().cpu() for k, v in m.state_dict().items()})
    noisy = spec.double().cpu().permute(0, 1, 3, 2, 4)           # [S, M, F, T, 2]
    ref = md._head_phi(xl.double().cpu().permute(0, 1, 3, 2), noisy)   # 2 x [S, F*T, 3, 3]
    for q in range(2):
        got = rows[q].cpu().double().view(B, F, Nc, T, 16).permute(2, 0, 1, 3, 4).reshape(S, F * T, 16)  # segment-major [n][b]
        assert torch.isfinite(got).all()
        assert torch.count_nonzero(got[..., 9:]) == 0
        want = ref[q].reshape(S, F * T, 9)
        assert rel_rms(got[..., :9].numpy(), want.numpy()) < 2e-6, q
        for f_, t_ in ((0, 0), (0, T - 1), (F - 1, 0), (F - 1, T - 1)):  # edge bins of every stream
            i = f_ * T + t_
            assert torch.allclose(got[:, i, :9], want[:, i], rtol=1e-4, atol=1e-4 * float(want.abs().max()))


@pytest.mark.parametrize("zero", [False, True])
@torch.no_grad()
def test_seq_kernel(zero):
    m = make_model("full")
    B, Nc, H = 2, 2, 256
    S = B * Nc
    h = [torch.zeros(B * F * Nc * T, H, device=DEV) if zero else rng_t(10 + q, B * F * Nc * T, H, scale=0.5) for q in range(2)]
    phi, ys, yn = (torch.empty(S, F, T, 9, device=DEV) for _ in range(3))
    sS, sN = m.gru_S, m.gru_N
    K._chk(K._lib().se_gbf_seq_fwd(_p(h[0]), _p(h[1]), _p(sS.fc_output_layer.weight), _p(sS.fc_output_layer.bias), _p(sS.norm.weight),
                                    _p(sS.norm.bias), _p(sN.fc_output_layer.weight), _p(sN.fc_output_layer.bias), _p(sN.norm.weight),
                                    _p(sN.norm.bias), _p(phi), _p(ys), _p(yn), S, B, F, T, H, K._st()))
    outs = []
    for q, sm in enumerate((sS, sN)):
        x = h[q].double().cpu().view(B, F, Nc, T, H).permute(2, 0, 1, 3, 4).reshape(S * F, T, H)   # segment-major sequences
        o = torch.relu(x @ sm.fc_output_layer.weight.double().cpu().t() + sm.fc_output_layer.bias.double().cpu())
        nrm = type("N", (), dict(weight=sm.norm.weight.double().cpu(), bias=sm.norm.bias.double().cpu()))
        outs.append(_gln(o.unsqueeze(1), nrm).squeeze(1).reshape(S, F, T, 9))
    for got, want in ((ys, outs[0]), (yn, outs[1]), (phi, outs[0] * outs[1])):
        assert torch.isfinite(got).all()
        assert rel_rms(got.cpu().numpy(), want.numpy()) < 2e-6


@pytest.mark.parametrize("zero", [False, True])
@torch.no_grad()
def test_bf_kernel(zero):
    m = make_model("full")
    S, H = 3, 256
    phi = torch.zeros(S, F, T, 9, device=DEV) if zero else rng_t(20, S, F, T, 9)
    spec = rng_t(21, S, M, T, F, 2, scale=3.0)
    Y = torch.empty(S, T, F, 2, device=DEV)
    w = torch.empty(S, F, T, 6, device=DEV)
    lin = m.linear
    K._chk(K._lib().se_gbf_bf_fwd(_p(phi), _p(spec), _p(lin[0].weight), _p(lin[0].bias), _p(lin[2].weight), _p(lin[2].bias), _p(lin[3].weight),
                                   _p(lin[3].bias), _p(Y), _p(w), S, M, T, F, H, K._st()))
    ld = make_model("full", "cpu").linear.double()
    ld.load_state_dict({k: v.double().cpu() for k, v in lin.state_dict().items()})
    wr = ld(phi.double().cpu())
    Yr = GeneralBeamformer._beamform(wr.reshape(S, F, T, M, 2), spec.double().cpu().permute(0, 1, 3, 2, 4))   # [S, F, T, 2]
    assert torch.isfinite(Y).all() and torch.isfinite(w).all()
    assert rel_rms(w.cpu().numpy(), wr.numpy()) < 1e-5
    assert rel_rms(Y.cpu().permute(0, 2, 1, 3).numpy(), Yr.numpy()) < 1e-5


# ---- the whole kernel path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_kernel_path_matches_reference_fixture(tag):
    gg = np.load(os.path.join(ROOT, "tests", "golden", "gbf_golden.npz"))
    m = make_model(tag)
    mix = mgb.mixture()
    with torch.no_grad():
        for c, (a, b, flag) in enumerate(mgb.CHUNKS):
            y = m.realtime_process(torch.from_numpy(mix[..., a:b].copy()).to(DEV), flag=flag).cpu().numpy()
            assert m._last_path == "kernel"
            assert rel_rms(y, gg[f"{tag}_out{c}"]) <= 1e-4, (tag, c, rel_rms(y, gg[f"{tag}_out{c}"]))


def _kernel_vs_restatement(tag, B, seconds_chunks):
    mk, mt = make_model(tag), make_model(tag)
    mt.use_hip_kernels(False)
    mt.spectrum = kernel_spectrum(mt)
    mix, _ = synth.synth_utterances(B, sum(seconds_chunks), 3, seed=23)
    a = 0
    with torch.no_grad():
        for c, n in enumerate(seconds_chunks):
            x = torch.from_numpy(mix[..., a:a + n].copy()).to(DEV)
            yk = mk.realtime_process(x, flag=c > 0)
            yt = mt.realtime_process(x, flag=c > 0)
            assert mt._last_path == "torch" and mk._last_path == "kernel"
            err = rel_rms(yk.cpu().numpy(), yt.cpu().numpy())
            assert err <= 1e-4, (tag, B, c, err)
            a += n


def test_kernel_path_matches_restatement_b8_3s():
    _kernel_vs_restatement("full", 8, [48000])


def test_flag_true_continuation_matches_restatement():
    _kernel_vs_restatement("full", 2, [11200, 6400, 8000])


def test_chunked_equals_unchunked_and_runs_are_bit_identical():
    m = make_model("full")
    mix = torch.from_numpy(synth.synth_utterances(2, 24000, 3, seed=31)[0]).to(DEV)
    with torch.no_grad():
        m.max_segments = 1000
        y_all = m.realtime_process(mix)
        y_all2 = m.realtime_process(mix)
        m.max_segments = 4
        y_4 = m.realtime_process(mix)
    assert torch.equal(y_all, y_all2)
    assert torch.equal(y_all, y_4)


def test_flag_true_with_another_batch_size_raises():
    m = make_model("tiny")
    mix = torch.from_numpy(synth.synth_utterances(2, 6400, 3, seed=3)[0]).to(DEV)
    with torch.no_grad():
        m.realtime_process(mix)
        with pytest.raises(ValueError, match="batch"):
            m.realtime_process(mix[:1], flag=True)


def test_unsupported_geometry_raises_on_the_gpu():
    m = GeneralBeamformer(**dict(mgb.TINY, hidden=24)).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="persistent GRU"):
        m.realtime_process(torch.zeros(1, 3, 3200, device=DEV))


def test_b64_completes_without_timeout():
    m = make_model("full")
    mix = torch.from_numpy(synth.synth_utterances(64, 48000, 3, seed=41)[0]).to(DEV)
    with torch.no_grad():
        y = m.realtime_process(mix)   # raises RuntimeError on a persistent-GRU timeout
    assert y.shape == (64, 48000) and torch.isfinite(y).all()
