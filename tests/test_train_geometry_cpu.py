"""CPU tests of train_stages.segment_geometry, the one statement of a realtime_process call's geometry on the kernel paths:
against bench.seg_count, against the torch restatement's segmentation (training._TrainableMixin._segment), and the U-Net frequency
sizes against the restatement's own encoder convolutions."""
import pytest
import torch
import torch.nn.functional as Fn

import bench
from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer
from speech_enhancement_mi_amd.train_stages import segment_geometry
from speech_enhancement_mi_amd.training import _TrainableMixin

KS = 3200
LENGTHS = [1, 799, 1600, 3199, 3200, 3201, 4800, 6400, 8000, 16000, 48000, 48001, 51199]   # 1 .. 3199: shorter than one segment
STFTS = [(400, 160), (512, 256)]   # (n_fft, hop): the 400-point and the 512-point geometry


class _Seg:
    segment_length = KS
    _segment = _TrainableMixin._segment


@pytest.mark.parametrize("n_fft,hop", STFTS)
@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
def test_segment_count_and_gap(L, flag, n_fft, hop):
    g = segment_geometry(L, flag, KS, hop, n_fft)
    P = KS // 2
    assert (g["Ks"], g["P"], g["T"], g["F0"]) == (KS, P, 1 + KS // hop, n_fft // 2 + 1)
    assert g["Lp"] - g["skip"] == L
    assert (g["off0"], g["skip"]) == ((-P, 0) if flag else (-2 * P, P))
    if not flag:
        assert g["N"] == bench.seg_count(L)
    x = torch.zeros(1, 1, L)
    seg, gap = _Seg()._segment(x if flag else Fn.pad(x, (P, 0)))   # the restatement pads P on the left for flag=False
    assert g["N"] == seg.shape[2] and g["gap"] == gap and seg.shape[3] == KS
    assert (g["Lp"] + g["gap"]) % P == 0 and 0 < g["gap"] <= KS


@pytest.mark.parametrize("n_fft,hop", STFTS)
def test_frequency_sizes_match_the_restatement_encoder(n_fft, hop):
    chans = [4, 8, 8, 8]
    m = GeneralBeamformer(num_channels=chans, num_freqs=n_fft // 2 + 1, hidden=16, segment_length=KS, num_layers=1, n_fft=n_fft,
                          hop_length=hop // 16, win_length=n_fft // 16)
    ch = [5] + chans
    g = segment_geometry(KS, False, KS, hop, n_fft, ch)
    assert g["ch"] == ch and len(g["Fq"]) == len(ch) and g["Fq"][0] == n_fft // 2 + 1
    h = torch.zeros(1, ch[0], g["F0"], g["T"])
    with torch.no_grad():
        for i, blk in enumerate(m.convlist):   # the restatement's convolution: [B, C, F, T], stride 2 over F, causal history over T
            h = blk.conv(Fn.pad(h, (blk.padding, 0)))
            assert tuple(h.shape) == (1, ch[i + 1], g["Fq"][i + 1], g["T"])
