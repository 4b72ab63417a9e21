"""The decoder's transposed convolutions above the last level run both output-frequency parities in ONE k_conv_p launch
(k_conv_p<9, NT, 1, PL, 6>: each chunk of the input patch is staged once for the 9 even and the 6 odd taps).  SE_DEC_PAIR=0 keeps
the two-launch form; both must give the same decoder levels and the same output."""
import numpy as np
import pytest
import torch

from conftest import FULL400, FULL512, STUDENT400
from engine_cases import cuda as _cuda, make_engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / (np.linalg.norm(b.ravel()) + 1e-30))


def _engine(cfg, monkeypatch, pair, variant=0, precision=0, seed=0):
    return make_engine(cfg, monkeypatch, {"SE_DEC_PAIR": "1" if pair else "0"}, variant=variant, precision=precision, seed=seed)


def _pair_vs_two_launches(monkeypatch, cfg, B, precision=0, variant=0, lengths=None, seed=0, pair_expected=True):
    a = _engine(cfg, monkeypatch, True, variant, precision, seed)
    b = _engine(cfg, monkeypatch, False, variant, precision, seed)
    n = max(lengths) if lengths else 6400
    mix, _ = synth.synth_utterances(B, n, cfg["num_inputs"], seed=seed + 11)
    ya = a.realtime_process(_cuda(mix), lengths=lengths).cpu().numpy()
    taps_a = [a.read_tap(f"dec{j}") for j in range(3)]
    yb = b.realtime_process(_cuda(mix), lengths=lengths).cpu().numpy()
    taps_b = [b.read_tap(f"dec{j}") for j in range(3)]
    # the R outputs are bit-identical (same K order per position); the statistics partials may be grouped differently, an fp32
    # rounding of the mean / variance, which the split into two bf16 planes (or one fp16 plane) can turn into one unit of that format
    tol = {0: 1e-6, 2: 1e-5, 1: 1e-4}[precision]
    for j in range(3):
        assert _rel(taps_a[j], taps_b[j]) <= tol, (j, _rel(taps_a[j], taps_b[j]))
    assert _rel(ya, yb) <= tol, _rel(ya, yb)
    # which form each engine launched: a pair launch is labelled dec<j>, the two-launch form dec<j>_even / dec<j>_odd.  The cost
    # model picks per level (the 512-point dec2 at B = 256 keeps two launches), so: each level one form, and some level paired
    la = _dec_labels(a, mix, lengths)
    npair = 0
    for j in range(3):
        lv = {x for x in la if x.startswith(f"dec{j}")}
        assert lv in ({f"dec{j}"}, {f"dec{j}_even", f"dec{j}_odd"}), la
        npair += lv == {f"dec{j}"}
    assert (npair > 0) == pair_expected, la
    assert _dec_labels(b, mix, lengths) == _TWO
    return a, mix, ya


_TWO = {f"dec{j}_{p}" for j in range(3) for p in ("even", "odd")}


def _dec_labels(e, mix, lengths):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # timed events: on a stream of their own (bench.py)
        e.profile(True)
        e.realtime_process(_cuda(mix), lengths=lengths)
        recs = e.profile_read()
        e.profile(False)
    torch.cuda.synchronize()
    return {r["label"] for r in recs if r["kernel"] == "k_conv_p" and r["label"].startswith("dec") and not r["label"].startswith("dec3")}


@pytest.mark.parametrize("B", [3, 256])
@pytest.mark.parametrize("precision", [0, 2])
def test_pair_launch_equals_two_launches(monkeypatch, B, precision):
    a, mix, ya = _pair_vs_two_launches(monkeypatch, FULL512, B, precision)
    # deterministic: no atomics, the statistics slab is summed in a fixed order
    a.reset(B)
    ya2 = a.realtime_process(_cuda(mix)).cpu().numpy()
    assert np.array_equal(ya, ya2)


@pytest.mark.parametrize("variant,cfg,precision", [(1, FULL400, 0), (2, STUDENT400, 2)])
def test_pair_launch_crn_elu_and_student(monkeypatch, variant, cfg, precision):
    _pair_vs_two_launches(monkeypatch, cfg, 5, precision, variant)


def test_fp16_operands_keep_two_launches(monkeypatch):
    """With one fp16 plane the decoder keeps one launch per parity (the pair launch measured slower there): SE_DEC_PAIR=1 and =0
    run the same code."""
    _pair_vs_two_launches(monkeypatch, STUDENT400, 5, 1, 2, pair_expected=False)


def test_pair_launch_ragged_batch(monkeypatch):
    """A ragged batch launches every segment for the prefix of streams still running (Bact < B)."""
    _pair_vs_two_launches(monkeypatch, FULL400, 6, lengths=[16000, 41234, 9600, 23999, 1, 3200])
