"""The distillation feature taps ft0, ft2.. re-run the plane path's own launches (k_conv_p without activation and statistics on the planes
still held in the ring slot, then k_tap_r_to_bcft).  The student goldens reach them at the TINY geometry only; here: the fp16 pair format and
four row tiles (FULL400), bf16 planes (SE_F16_PAIR=0), the R-layout twin of the student's last encoder plan (STUDENT400) and one
padded octet (TINY, CRN).  Every case: two streams, a reset, half-overlapping segments, so that ft0 convolves real history."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from conftest import FULL400, STUDENT400, TINY, rel_rms, spec_of_variant
from engine_cases import cuda as _cuda, make_engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TOL_TAP = 2e-5  # the project's tap bar (test_student_feature_taps_golden, test_gpu_fc_gln_fused.TOL_TAP)
B = 2


def _engine(cfg, seed):
    sd = synth.make_state_dict(spec_of_variant(cfg, 0), seed=seed)
    return make_engine(cfg, sd=sd), sd


@pytest.mark.parametrize("case", ["full400", "full400_bf16", "tiny"])
def test_crn_feature_taps_equal_float64_convolutions_of_the_operand_taps(case, monkeypatch):
    """Variant 0.  The reference is float64 torch on the CPU, computed from the engine's OWN operand taps (the plane sums the re-run
    reads), so the bar measures the re-run alone:
      ft0      = conv2d of [last 2 * 2^(L-1) frames of segment 0's enc<L-2> | segment 1's enc<L-2>] with convlist.<L-1>.conv,
                 stride (2, 1), frequency padding 2, time dilation 2^(L-1)                                      (CRN.py:331-336)
      ft<2+j>  = conv_transpose2d of gru / dec<j-1> with deconvlist.<j>.conv, the last T frames                    (CRN.py:383-386)
    and the device form (se_read_tap_dev) is bit-equal to the host form."""
    cfg = TINY if case == "tiny" else FULL400
    if case == "full400_bf16":
        monkeypatch.setenv("SE_F16_PAIR", "0")
    e, sd = _engine(cfg, seed=3)
    ch, L, K = cfg["num_channels"], len(cfg["num_channels"]), cfg["segment_length"]
    Fq = [cfg["num_freqs"]]
    for _ in range(L):
        Fq.append((Fq[-1] - 1) // 2 + 1)
    mix, _ = synth.synth_utterances(B, K + K // 2, 3, seed=41)
    e.reset(B)
    e.step(_cuda(mix[:, :, :K]))
    enc_prev = e.read_tap(f"enc{L - 2}").reshape(B, ch[L - 2], Fq[L - 1], -1)
    e.step(_cuda(mix[:, :, K // 2:]))
    T = enc_prev.shape[-1]
    tap = lambda name, C, F: torch.from_numpy(e.read_tap(name).reshape(B, C, F, T)).double()
    w = lambda key: torch.from_numpy(sd[key]).double()
    d = 2 ** (L - 1)
    inp = torch.cat([torch.from_numpy(enc_prev[..., -2 * d:]).double(), tap(f"enc{L - 2}", ch[L - 2], Fq[L - 1])], dim=-1)
    refs = {0: Fn.conv2d(inp, w(f"convlist.{L - 1}.conv.weight"), w(f"convlist.{L - 1}.conv.bias"), stride=(2, 1), padding=(2, 0), dilation=(1, d))}
    for j in range(L - 1):
        x = tap("gru", ch[L - 1], Fq[L]) if j == 0 else tap(f"dec{j - 1}", ch[L - 1 - j], Fq[L - j])
        refs[2 + j] = Fn.conv_transpose2d(x, w(f"deconvlist.{j}.conv.weight"), w(f"deconvlist.{j}.conv.bias"), stride=(2, 1), padding=(2, 0),
                                          dilation=(1, 2 ** j))[..., -T:]
    for k, ref in refs.items():
        host = e.read_tap(f"ft{k}")
        assert host.size == ref.numel(), (k, host.size, tuple(ref.shape))
        r = rel_rms(host.reshape(ref.shape), ref.numpy())
        print(f"{case} ft{k} {tuple(ref.shape)}: rel rms {r:.3e}")
        assert r < TOL_TAP, (case, k, r)
        assert np.array_equal(e.read_tap_dev(f"ft{k}", host.size).cpu().numpy(), host), k


def test_student400_feature_taps_equal_the_torch_restatement():
    """Variant 2 at the full student geometry: the five maps of distillation_crn.TemporalCRN.realtime_process (one se_step and five
    se_read_tap_dev per segment) against the project's torch restatement on the CPU, realtime_process_train(..., features=True), which the
    goldens pin to the genuine reference.  A fresh call's first window is all padding; the bar is on the windows that hold signal, and the
    last one's ft0 has a signal window as its history."""
    from speech_enhancement_mi_amd.distillation_crn import TemporalCRN as Student
    from speech_enhancement_mi_amd.training import TrainableStudentCRN
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of_variant(STUDENT400, 2), seed=1).items()}
    ref_m = TrainableStudentCRN(**STUDENT400)
    ref_m.load_state_dict(sd, strict=True)
    m = Student(**STUDENT400)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    mix, _ = synth.synth_utterances(B, 3200, 3, seed=43)
    with torch.no_grad():
        _, ref = ref_m.realtime_process_train(torch.from_numpy(mix), features=True)
    _, feats = m.realtime_process(_cuda(mix))
    assert len(feats) == 5 and ref[0].shape[0] >= 3 * B  # at least two windows with signal
    for k, (f, r) in enumerate(zip(feats, ref)):
        assert tuple(f.shape) == tuple(r.shape), (k, f.shape, r.shape)
        err = rel_rms(f[B:].cpu().numpy(), r[B:].numpy())
        print(f"student400 ft{k} {tuple(r.shape)}: rel rms {err:.3e}")
        assert err < TOL_TAP, (k, err)
