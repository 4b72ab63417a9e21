"""The two ends of a segment run as fused kernels (csrc/io_fused.hip.h): k_stft_feat = k_stft of all microphones + k_featurize_p,
k_mask_istft = k_final_mask_p + k_istft.  SE_IO_FUSE=0 keeps the four-kernel route.  The fused kernels run the same butterflies, feature
and mask expressions on the same data, so every comparison here is for the same bits."""
import numpy as np
import pytest
import torch

from conftest import TINY
from engine_cases import cuda as _cuda, make_engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TINY512 = dict(TINY, num_freqs=257, n_fft=512)
CFGS = [pytest.param(TINY, id="400"), pytest.param(TINY512, id="512")]


def _engine(cfg, monkeypatch, fuse, variant=0, precision=0, pipeline=None, seed=0):
    env = {} if fuse else {"SE_IO_FUSE": "0"}  # the default engine is made with nothing set
    if pipeline is not None:
        env["SE_PIPELINE"] = str(pipeline)
    return make_engine(cfg, monkeypatch, env, variant=variant, precision=precision, seed=seed)


def _pair(cfg, monkeypatch, **kw):
    return _engine(cfg, monkeypatch, False, **kw), _engine(cfg, monkeypatch, True, **kw)


def _same(ref, new, mix, **kw):
    """feat tap (of the last segment) and output of one call on both engines: the same bits"""
    x = _cuda(mix)
    yr = ref.realtime_process(x, **kw).cpu().numpy()
    fr = ref.read_tap("feat")
    yn = new.realtime_process(x, **kw).cpu().numpy()
    fn = new.read_tap("feat")
    assert np.isfinite(yr).all() and np.abs(yr).max() > 0
    assert np.array_equal(fr, fn), float(np.abs(fr - fn).max())
    assert np.array_equal(yr, yn), float(np.abs(yr - yn).max())
    return yr, fr


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("cfg", CFGS)
def test_fused_equals_four_kernels(monkeypatch, cfg, pipeline):
    """B = 3, 11 200 samples: the first and the last segment are partly zero fill; then a continuing call (flag=True) on 6 400."""
    ref, new = _pair(cfg, monkeypatch, pipeline=pipeline)
    mix, _ = synth.synth_utterances(3, 11200 + 6400, cfg["num_inputs"], seed=21)
    _same(ref, new, mix[:, :, :11200])
    _same(ref, new, mix[:, :, 11200:], flag=True)


@pytest.mark.parametrize("cfg", CFGS)
def test_fused_ragged_batch(monkeypatch, cfg):
    """Per-stream lengths and offsets (Lrow, offrow) and a launch batch that shrinks (Bact < B)."""
    lengths = [16000, 41234, 9600, 23999, 1, 3200]
    ref, new = _pair(cfg, monkeypatch)
    mix, _ = synth.synth_utterances(6, max(lengths), cfg["num_inputs"], seed=22)
    _same(ref, new, mix, lengths=lengths)


@pytest.mark.parametrize("variant,precision", [(1, 1), (2, 0)])
def test_fused_crn_elu_and_student(monkeypatch, variant, precision):
    """CRN_ELU with fp16 operands: the pre-conv blocks run on the plane path and k_stft_feat writes their input (atan2 phase).  The
    student at default precision keeps k_stft for its fp32 pre-conv blocks: only the mask side fuses."""
    ref, new = _pair(TINY, monkeypatch, variant=variant, precision=precision)
    mix, _ = synth.synth_utterances(3, 11200, TINY["num_inputs"], seed=23)
    _same(ref, new, mix)
    want = {"stft_feat", "mask_istft"} if variant == 1 else {"stft", "featurize", "mask_istft"}
    assert _io_labels(new, mix) == want


@pytest.mark.parametrize("cfg", CFGS)
def test_fused_silent_stream(monkeypatch, cfg):
    """An all-zero stream next to a non-zero one: each frame is transformed on its own, so the silent stream's spectra are exact
    zeros, and its features and output are those of the four-kernel route bit for bit."""
    ref, new = _pair(cfg, monkeypatch)
    mix, _ = synth.synth_utterances(3, 11200, cfg["num_inputs"], seed=24)
    mix[1] = 0.0
    _, feat = _same(ref, new, mix)
    M = cfg["num_inputs"]
    silent = feat.reshape(3, 2 * M - 1, -1)[1]
    assert np.all(silent[:M] == silent[0, 0]) and abs(float(silent[0, 0]) - 1e-5) < 1e-10  # sqrt(0 + 1e-10): magnitudes of exact zeros
    assert np.all(silent[M:] == 0.0)                                                        # and equal phases


_IO = {"stft", "istft", "featurize", "final_mask", "stft_feat", "mask_istft"}


def _io_labels(e, mix):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # timed events: on a stream of their own (bench.py)
        e.profile(True)
        e.realtime_process(_cuda(mix))
        recs = e.profile_read()
        e.profile(False)
    torch.cuda.synchronize()
    return {r["label"] for r in recs} & _IO


def test_profile_records(monkeypatch):
    ref, new = _pair(TINY512, monkeypatch)
    mix, _ = synth.synth_utterances(3, 6400, 3, seed=25)
    assert _io_labels(new, mix) == {"stft_feat", "mask_istft"}
    assert _io_labels(ref, mix) == {"stft", "featurize", "final_mask", "istft"}
