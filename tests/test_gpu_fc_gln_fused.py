"""The bottleneck's output norm on the plane GEMM route: the fc_output_layer weight rows (and the norm's per-element affine) are
permuted at load time so that the GEMM writes octet-interleaved columns, k_gemm_p's epilogue leaves one (sum, sum of squares) pair per
row and column tile, and k_gln2_p is a full-chip one-pass kernel.  Checked against the C oracle at the bars the parity tests
hold each precision to: fp32 taps 2e-5 / output 1e-4, bf16x3 output 1e-4, fp16 output 3e-3 of the fp32 engine.

SE_GEMM_SKINNY_ROWS=0 (read when the engine is created) sends batches of any size down the plane GEMM route, so the shapes here
stay small: B = 13 x T = 21 = 273 GEMM rows is the smallest batch whose rows cross a 256-row tile (stream 12 straddles two row
tiles and the last tile is mostly padding); B = 1 is a single partial tile."""
import functools

import numpy as np
import pytest
import torch

from conftest import FULL400, FULL512, STUDENT400, rel_rms, spec_of_variant
from engine_cases import cuda as _cuda, make_engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TOL, TOL_TAP, TOL_F16 = 1e-4, 2e-5, 3e-3
CASES = {"crn512": (FULL512, 0), "crn400": (FULL400, 0), "elu400": (FULL400, 1), "student400": (STUDENT400, 2)}
PICK = [0, 11, 12]  # streams the oracle restates: first tile, last whole stream of row tile 0, the stream that straddles the tiles


def _state_dict(cfg, variant):
    """Hash weights, with the norm behind fc_output_layer given an affine that is distinct in every element and varies by the same
    order along c and along f: a transposed (c, f) <-> (f, c) permutation cannot hide behind it."""
    sd = dict(synth.make_state_dict(spec_of_variant(cfg, variant), seed=3))
    shape = np.asarray(sd["gru.norm.weight"]).shape  # D elements, d = c * F + f, whatever the singleton axes around them
    D = int(np.prod(shape))
    k = np.arange(D, dtype=np.float64)
    sd["gru.norm.weight"] = (0.5 + ((k * 37) % D) / D).astype(np.float32).reshape(shape)
    sd["gru.norm.bias"] = (((k * 101) % D) / D - 0.5).astype(np.float32).reshape(shape)
    assert len(np.unique(sd["gru.norm.weight"])) == D and len(np.unique(sd["gru.norm.bias"])) == D
    return sd


def _engine(monkeypatch, case, precision=0):
    cfg, variant = CASES[case]
    return make_engine(cfg, monkeypatch, {"SE_GEMM_SKINNY_ROWS": "0"}, variant=variant, precision=precision, sd=_state_dict(cfg, variant))


def _oracle(case):
    from oracle import crn_oracle as orc
    cfg, variant = CASES[case]
    o = orc.CrnOracle(**cfg, variant=variant)
    o.load_state_dict(_state_dict(cfg, variant))
    return o


@functools.lru_cache(maxsize=None)
def _reference(case):
    """One segment of 13 streams; the oracle's decoder input and output for the streams in PICK (streams are independent).
    Computed once per geometry and shared; the arrays are read-only."""
    cfg, _ = CASES[case]
    o = _oracle(case)
    mix, _ = synth.synth_utterances(13, 3200, 3, seed=29)
    x = o.stft(mix.reshape(-1, 3200)).reshape(13, 3, cfg["num_freqs"], 21, 2)
    o.reset(len(PICK))
    y = np.array(o.forward(np.ascontiguousarray(x[PICK])))
    tap = np.array(o.tap("gru")).reshape(len(PICK), -1)
    for a in (x, y, tap):
        a.setflags(write=False)
    return x, y, tap


def _forward(e, x):
    e.reset(x.shape[0])
    y = e.forward(_cuda(x)).cpu().numpy()
    return y, e.read_tap("gru").reshape(x.shape[0], -1)


def _norm_kernels(e, x):
    """Which gLN kernel of the fc output the engine launches for this batch."""
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # timed events: on a stream of their own (bench.py)
        e.profile(True)
        e.forward(_cuda(x))
        recs = e.profile_read()
        e.profile(False)
    torch.cuda.synchronize()
    return {r["kernel"] for r in recs if r["label"].startswith("gln_fc")}


@pytest.mark.parametrize("case", list(CASES))
def test_row_tile_straddle_vs_oracle(monkeypatch, case):
    """B = 13: 273 GEMM rows, two row tiles.  512-pt CRN (C = 128, F = 17), 400-pt CRN and CRN_ELU (another F; T * F is no
    multiple of the block), student (C = 64, hidden 128).  The affine is distinct per element, so the decoder-input tap in the
    reference's order pins the load-time permutation."""
    x, yo, tapo = _reference(case)
    e = _engine(monkeypatch, case)
    y, tap = _forward(e, x)
    assert _norm_kernels(e, x) == {"k_gln2_p"}
    assert np.array_equal(_forward(e, x)[0], y)  # no atomics: a second run is bit-identical
    for i, b in enumerate(PICK):
        r = rel_rms(tap[b], tapo[i])
        print(case, "stream", b, "decoder-input tap", r, "output", rel_rms(y[b], yo[i]))
        assert r < TOL_TAP, (case, b, r)
        assert rel_rms(y[b], yo[i]) < TOL, (case, b)


@pytest.mark.parametrize("case", ["crn512", "student400"])
def test_single_stream_partial_tile(monkeypatch, case):
    """B = 1: 21 rows of one 256-row tile."""
    x, yo, tapo = _reference(case)
    e = _engine(monkeypatch, case)
    y, tap = _forward(e, np.ascontiguousarray(x[:1]))
    assert _norm_kernels(e, np.ascontiguousarray(x[:1])) == {"k_gln2_p"}
    r = rel_rms(tap[0], tapo[0])
    print(case, "decoder-input tap", r, "output", rel_rms(y[0], yo[0]))
    assert r < TOL_TAP, r
    assert rel_rms(y[0], yo[0]) < TOL


@pytest.mark.parametrize("case", ["crn512", "student400"])
def test_bf16x3_and_fp16(monkeypatch, case):
    """bf16x3 (two planes) at the fp32 bar on the output; fp16 operands within 3e-3 of the fp32-accurate engine."""
    x, yo, _ = _reference(case)
    y32, _ = _forward(_engine(monkeypatch, case, 0), x)
    y3, _ = _forward(_engine(monkeypatch, case, 2), x)
    y16, _ = _forward(_engine(monkeypatch, case, 1), x)
    for i, b in enumerate(PICK):
        print(case, "stream", b, "bf16x3 vs oracle", rel_rms(y3[b], yo[i]))
        assert rel_rms(y3[b], yo[i]) < TOL, (case, b)
    print(case, "fp16 vs fp32 engine", rel_rms(y16, y32))
    assert np.isfinite(y16).all() and rel_rms(y16, y32) < TOL_F16


def test_default_route_small_batch_unchanged(monkeypatch):
    """Without the override a batch of 13 streams stays on the fp32 GEMM route (reference column order, two-pass statistics)."""
    cfg, variant = CASES["crn400"]
    x, yo, tapo = _reference("crn400")
    e = make_engine(cfg, variant=variant, sd=_state_dict(cfg, variant))
    y, tap = _forward(e, x)
    assert _norm_kernels(e, x) == {"k_gln2_stream_p"}
    for i, b in enumerate(PICK):
        assert rel_rms(tap[b], tapo[i]) < TOL_TAP and rel_rms(y[b], yo[i]) < TOL, b


def test_ragged_prefix_and_determinism(monkeypatch):
    """se_realtime_process_ragged with lengths that retire streams early (Bact < B in the later segments): rows of retired streams
    are neither written nor read, so every stream equals the oracle's run of that stream alone, at the output bar of the
    other cases.  The samples beyond each stream's length are large garbage: a dead row that reached any statistics would show.
    Two runs are bit-identical: the slab is written once per slot and summed in a fixed order."""
    case = "crn400"
    lengths = [8000, 8000, 6400, 4800] + [3200] * 5 + [1600, 1600, 700, 1]
    mix, _ = synth.synth_utterances(13, 8000, 3, seed=31)
    clean = mix.copy()
    for b, n in enumerate(lengths):
        mix[b, :, n:] = 1e3 * (1 + b)
    e = _engine(monkeypatch, case)
    y = e.realtime_process(_cuda(mix), lengths=lengths).cpu().numpy()
    y2 = e.realtime_process(_cuda(mix), lengths=lengths).cpu().numpy()
    assert np.array_equal(y, y2)
    o = _oracle(case)
    for b in (0, 3, 12):
        n = lengths[b]
        ref = np.asarray(o.realtime_process(np.ascontiguousarray(clean[b:b + 1, :, :n])))[0]
        err = rel_rms(y[b, :n], ref)
        print("stream", b, "length", n, "rel rms error", err)
        assert err < TOL, (b, err)
