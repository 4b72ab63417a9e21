"""se_realtime_process_chains on the GPU: B chunk chains in one call, each stream with its own length and its own flag, each leaving
exactly the state it would carry alone (DESIGN.md 6 "Batched chunk chains", restated for the inference engine)."""
import functools

import numpy as np
import pytest
import torch

import chain_cases as cc
from conftest import FULL400, TINY, rel_rms
from engine_cases import cuda as _cuda, make_engine as _engine
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd.engine import chain_geometry

pytestmark = pytest.mark.gpu

K_RING = 4            # csrc/se_engine.hip kRing: activation ring slots
BAR_ALONE = 2e-6      # batch against each stream alone: the bar of test_gpu_round3.py::test_ragged_batch_equals_each_stream_alone
# bf16x3 (precision 2), batch against alone.  The bar is twice what the parent commit measures for case 2's call 1 through
# se_realtime_process_ragged against every stream alone at precision 2: measured 0.0 for every stream (MI355X; batch 6 and batch 1 take
# the same kernels and tilings, rows are independent) -> the bar is bit equality.  The uniform case of the parent (6 equal streams of
# 60000 then 48000 samples, flag=False then flag=True, batch against alone) measures 0.0 / 0.0 as well, so BAR_ALONE needs no
# allowance for two calls accumulating.
BAR_BF16X3 = 2 * 0.0


# ---- 1. the reference fixture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["1", "0"], ids=["pipelined", "serial"])
@pytest.mark.parametrize("tag,variant", cc.VARIANTS)
def test_chains_match_the_reference_fixture(tag, variant, pipeline, monkeypatch):
    """The two calls of chain_cases.CALLS through Engine.realtime_process with per-stream flags: every utterance equals what the genuine
    reference gives for it ALONE (crn_chain_golden.npz), zeros beyond its length.  Call 1 runs 8 / 6 / 6 segments: utterance 2 ends early
    and continues in call 2 (a missing freeze fails), utterance 1 is reset among continuing streams (collapsed flags fail)."""
    monkeypatch.setenv("SE_PIPELINE", pipeline)
    g = cc.chain_golden()
    e = _engine(TINY, variant=variant, seed=0)
    assert chain_geometry(cc.CALLS[0][1], cc.CALLS[0][0], TINY["segment_length"])["Nb"] == [8, 6, 6]
    for c, (flags, lens) in enumerate(cc.CALLS):
        y = e.realtime_process(cc.chain_batch(c).cuda(), flag=list(flags), lengths=list(lens)).cpu().numpy()
        for b, l in enumerate(lens):
            err = rel_rms(y[b, :l], g[f"{tag}_call{c + 1}_utt{b}"])
            print(f"fixture {tag} pipeline={pipeline} call {c + 1} utt {b}: rel rms {err:.3e}")
            assert err < 1e-4, (tag, c, b, err)
            assert np.all(y[b, l:] == 0.0), (tag, c, b)


# ---- 2. each stream equals its own chain alone, ring reuse included ----------------------------------------------------------------
CASE2 = (([16000, 41234, 60000, 23999, 1, 3200], [0, 0, 0, 0, 0, 0]),
         ([9000, 30000, 5000, 48000, 20000, 1], [1, 0, 1, 1, 1, 0]),
         ([3200] * 6, [1, 1, 0, 1, 1, 1]))
PAD2 = 7.0


def _case_batches(calls, seed, pad):
    xs = []
    for c, (lens, _) in enumerate(calls):
        mix, _ = synth.synth_utterances(len(lens), max(lens), 3, seed=seed + c)
        for b, l in enumerate(lens):
            mix[b, :, l:] = pad
        xs.append(mix)
    return xs


def _state_names(cfg):
    return ["h"] + [f"buf{i}" for i in range(len(cfg["num_channels"]))]


def _run_batch(calls, xs, precision=0, export_after=None):
    e = _engine(FULL400, precision=precision, seed=4)
    ys, state = [], None
    for c, (lens, flags) in enumerate(calls):
        ys.append(e.realtime_process(_cuda(xs[c]), flag=[bool(f) for f in flags], lengths=lens).cpu())
        if c == export_after:
            state = {n: e.export_state(n) for n in _state_names(FULL400)}
    return ys, state


def _run_alone(calls, xs, streams, precision=0, export_after=None):
    """every listed stream's chain by itself on one batch-1 engine -> ys[c][b], state[b][name]"""
    e1 = _engine(FULL400, precision=precision, seed=4)
    ys, state = [dict() for _ in calls], {}
    for b in streams:
        for c, (lens, flags) in enumerate(calls):
            ys[c][b] = e1.realtime_process(_cuda(xs[c][b:b + 1, :, :lens[b]]), flag=bool(flags[b])).cpu().numpy()[0]
            if c == export_after:
                state[b] = {n: e1.export_state(n) for n in _state_names(FULL400)}
    return ys, state


@functools.lru_cache(maxsize=None)
def _case2(precision=0, ncalls=3):
    calls = CASE2[:ncalls]
    xs = _case_batches(calls, 60, PAD2)
    ys, state = _run_batch(calls, xs, precision, export_after=1)
    ys1, state1 = _run_alone(calls, xs, range(6), precision, export_after=1)
    return calls, ys, state, ys1, state1


def _check_outputs(calls, ys, ys1, streams, bar, what):
    for c, (lens, _) in enumerate(calls):
        y = ys[c].numpy()
        for b in streams:
            l = lens[b]
            err = rel_rms(y[b, :l], ys1[c][b])
            print(f"{what} call {c + 1} stream {b} (length {l}): rel rms {err:.3e}")
            assert (err < bar if bar > 0 else err == 0.0) or l == 1, (what, c, b, l, err)   # one sample: exempt from the ratio, as in test_ragged_batch_equals_each_stream_alone
            assert np.all(y[b, l:] == 0.0), (what, c, b)


def test_each_stream_equals_its_own_chain_alone():
    """FULL400, 6 streams, three calls (CASE2: lengths, flags), 7.0 beyond every length; one engine at batch 6 against one engine at
    batch 1 that runs every stream's chain by itself.  Output per call and stream, and after call 2 the exported h and conv buffers
    row by row.  Call 1 runs 14 / 28 / 40 / 18 / 4 / 6 segments: every early stream ends at least kRing + 2 segments before the
    longest one, so its state must have been saved when it ended (the ring has moved on).  (No stream of these lengths ends exactly two
    segments before the longest; that neighbourhood is asserted in the fixture case, 8 / 6 / 6, and in the compaction case.)"""
    calls, ys, state, ys1, state1 = _case2()
    nb = chain_geometry(calls[0][0], calls[0][1], FULL400["segment_length"])["Nb"]
    assert nb == [14, 28, 40, 18, 4, 6] and all(max(nb) - n >= K_RING + 2 for n in nb if n != max(nb))
    _check_outputs(calls, ys, ys1, range(6), BAR_ALONE, "case 2")
    B = 6
    for name in _state_names(FULL400):
        rows = state[name].reshape((FULL400["num_layers"], B, -1) if name == "h" else (B, -1))
        for b in range(B):
            got = rows[:, b].reshape(-1) if name == "h" else rows[b]
            ref = state1[b][name].reshape(-1)
            if not np.any(ref):
                assert np.max(np.abs(got)) <= 1e-6, (name, b)
                continue
            err = rel_rms(got, ref)
            print(f"case 2 state {name} stream {b} after call 2: rel rms {err:.3e}")
            assert err < BAR_ALONE, (name, b, err)


# ---- 3. the compaction route ----------------------------------------------------------------------------------------------------
CASE3_STREAMS = (0, 7, 13, 20, 33, 47)


def _case3_calls():
    B = 48
    rng = np.random.default_rng(5)
    l1 = [int(v) for v in rng.integers(16000, 32001, B)]
    l1[7], l1[20] = 32000, 16000
    l2 = [int(v) for v in rng.integers(16000, 32001, B)]
    f2 = [0 if b % 3 == 0 else 1 for b in range(B)]
    return ((l1, [0] * B), (l2, f2))


@functools.lru_cache(maxsize=None)
def _case3():
    calls = _case3_calls()
    xs = _case_batches(calls, 70, -3.0)
    ys, _ = _run_batch(calls, xs)
    ys1, _ = _run_alone(calls, xs, CASE3_STREAMS)
    return calls, ys, ys1


def test_compaction_route_keeps_every_stream_its_chain():
    """48 streams (the plane-GEMM route, where the shim's sort by segment count lets the engine launch prefixes): call 1 fresh, call 2 with
    every third stream reset and new lengths.  Six streams of both calls against their chains alone; outputs come back in the caller's
    order although the engine's slots are sorted (the slot map)."""
    calls, ys, ys1 = _case3()
    nb = chain_geometry(calls[0][0], calls[0][1], FULL400["segment_length"])["Nb"]
    assert sorted(nb, reverse=True) != nb and (max(nb) - 2) in nb   # unsorted as given; some stream ends two segments before the longest
    _check_outputs(calls, ys, ys1, CASE3_STREAMS, BAR_ALONE, "case 3")


# ---- 4. uniform batches are untouched; results are reproducible -------------------------------------------------------------------------
def test_uniform_batch_is_se_realtime_process():
    ea, eb = _engine(FULL400, seed=4), _engine(FULL400, seed=4)
    mix, _ = synth.synth_utterances(3, 2 * 9000, 3, seed=81)
    for c, flag in enumerate((False, True)):
        x = _cuda(mix[:, :, c * 9000:(c + 1) * 9000])
        ya = ea.realtime_process_chains(x, [flag] * 3, [9000] * 3)
        yb = eb.realtime_process(x, flag=flag)
        assert torch.equal(ya, yb), flag
        assert np.array_equal(ea.export_state("h"), eb.export_state("h")), flag


def test_chains_are_reproducible():
    calls, ys, state, _, _ = _case2()
    ys_b, state_b = _run_batch(calls, _case_batches(calls, 60, PAD2), export_after=1)
    for a, b in zip(ys, ys_b):
        assert torch.equal(a, b)
    for n in state:
        assert np.array_equal(state[n], state_b[n]), n
    calls3, ys3, _ = _case3()
    ys3_b, _ = _run_batch(calls3, _case_batches(calls3, 70, -3.0))
    for a, b in zip(ys3, ys3_b):
        assert torch.equal(a, b)


# ---- 5. bf16x3 ------------------------------------------------------------------------------------------------------------------
def test_chains_bf16x3():
    calls, ys, _, ys1, _ = _case2(precision=2, ncalls=2)
    _check_outputs(calls, ys, ys1, range(6), BAR_BF16X3, "bf16x3")


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------
def test_chain_errors_leave_the_engine_usable():
    e = _engine(TINY, seed=0)
    x = cc.chain_batch(0).cuda()
    lens = list(cc.CALLS[0][1])
    with pytest.raises(RuntimeError, match="carries no state"):
        e.realtime_process(x, flag=[True, False, False], lengths=lens)
    ref = e.realtime_process(x, flag=[False] * 3, lengths=lens).clone()
    with pytest.raises(RuntimeError, match="carried state holds 3 streams"):
        e.realtime_process(x[:2].contiguous(), flag=[True, False], lengths=lens[:2])
    with pytest.raises(RuntimeError, match="outside"):
        e.realtime_process(x, flag=[True, False, True], lengths=[lens[0], 0, lens[2]])
    with pytest.raises(RuntimeError, match="outside"):
        e.realtime_process(x, flag=[True, False, True], lengths=[lens[0], x.shape[2] + 1, lens[2]])
    with pytest.raises(RuntimeError, match="flags for a batch"):
        e.realtime_process(x, flag=[True, False], lengths=lens)
    with pytest.raises(RuntimeError, match="lengths for a batch"):
        e.realtime_process(x, flag=[True, False, True], lengths=lens[:2])
    # none of the refused calls touched the carried state: call 2 of the fixture still comes out right, and a fresh call repeats call 1
    g = cc.chain_golden()
    flags2, lens2 = cc.CALLS[1]
    y2 = e.realtime_process(cc.chain_batch(1).cuda(), flag=list(flags2), lengths=list(lens2)).cpu().numpy()
    for b, l in enumerate(lens2):
        assert rel_rms(y2[b, :l], g[f"crn_call2_utt{b}"]) < 1e-4, b
    assert torch.equal(e.realtime_process(x, flag=[False] * 3, lengths=lens), ref)


# ---- 7. a ragged call is a chains call; one signal chain; FullSubNet's frame floor ----------------------------------------------------
def test_ragged_call_is_a_chains_call_state_included():
    """se_realtime_process_ragged, called directly, against realtime_process(flag=[False] * 3, lengths=...) on a second engine with the
    same weights (TINY, the fresh batch of chain_cases.CALLS[0]): the same outputs and the same exported h / conv buffers, bit for bit -
    the streams that ended early keep their own state.  Then a flag=True call with the CALLS[1] lengths on the first engine: every
    stream within BAR_ALONE of its own two-chunk chain run alone."""
    import ctypes as C
    ea, eb, e1 = _engine(TINY, seed=0), _engine(TINY, seed=0), _engine(TINY, seed=0)
    lens0, lens1 = list(cc.CALLS[0][1]), list(cc.CALLS[1][1])
    x0, x1 = cc.chain_batch(0).cuda(), cc.chain_batch(1).cuda()
    B, L0 = x0.shape[0], x0.shape[2]
    ya = torch.empty((B, L0), dtype=torch.float32, device="cuda")
    ea._check(ea.lib.se_realtime_process_ragged(ea._h, ea._dev(x0), B, L0, (C.c_int64 * B)(*lens0), 0, ea._dev(ya, (B, L0)), ea._stream()))
    ea.batch = B
    yb = eb.realtime_process(x0, flag=[False] * B, lengths=lens0)
    assert np.array_equal(ya.cpu().numpy(), yb.cpu().numpy())
    for name in _state_names(TINY):
        assert np.array_equal(ea.export_state(name), eb.export_state(name)), name
    y2 = ea.realtime_process(x1, flag=True, lengths=lens1).cpu().numpy()
    for b in range(B):
        e1.realtime_process(x0[b:b + 1, :, :lens0[b]].contiguous(), flag=False)
        alone = e1.realtime_process(x1[b:b + 1, :, :lens1[b]].contiguous(), flag=True).cpu().numpy()[0]
        err = rel_rms(y2[b, :lens1[b]], alone)
        print(f"ragged continuation stream {b} (length {lens1[b]}): rel rms {err:.3e}")
        assert err < BAR_ALONE, (b, err)
        assert np.all(y2[b, lens1[b]:] == 0.0), b


@pytest.mark.parametrize("n_fft", [400, 512])
def test_engine_and_training_handle_share_one_signal_chain(n_fft):
    """Engine.stft / istft (se_stft, se_istft) and the training signal handle (train_stages._sig + se_sig_stft / se_sig_istft) on the same
    6 rows of 3200 samples: one table builder and one launcher behind both, so after the layout transpose the results are bit-equal."""
    from speech_enhancement_mi_amd import train_stages as ts
    from speech_enhancement_mi_amd import train_ops as K
    cfg = dict(TINY, n_fft=n_fft, num_freqs=n_fft // 2 + 1)
    e = _engine(cfg)
    c = e.cfg
    n, Ks = 6, cfg["segment_length"]
    seg = torch.from_numpy(np.random.default_rng(9).standard_normal((n, Ks)).astype(np.float32)).cuda()
    sig = ts._sig(seg.device, n_fft, c.win, c.hop, Ks)
    spec_e = e.stft(seg)                                                        # [n, F, T, 2]
    spec_s = ts._stft(sig, seg.reshape(n, 1, Ks), n, 1, Ks, 0, Ks // 2, 1, e.T, e.F)[0]   # [n, T, F, 2]
    assert np.array_equal(spec_e.permute(0, 2, 1, 3).cpu().numpy(), spec_s.cpu().numpy())
    assert float(spec_s.abs().max()) > 1.0
    wav_e = e.istft(spec_e)
    wav_s = torch.empty((n, Ks), dtype=torch.float32, device="cuda")
    K._chk(K._lib().se_sig_istft(sig, ts._p(spec_s.contiguous()), n, ts._p(wav_s), K._st()))
    assert np.array_equal(wav_e.cpu().numpy(), wav_s.cpu().numpy())
    assert rel_rms(wav_s.cpu().numpy(), seg.cpu().numpy()) < 1e-4   # sanity only: the pair inverts, so neither side compared empty buffers


@pytest.mark.parametrize("frames", [16, 2])
def test_fsn_engine_refuses_segments_of_at_most_16_frames(frames):
    """FsnEngine with a segment of at most 16 frames (segment_length <= 15 hops; 16 hops = 17 frames is the first accepted, before and
    after the engine got its own signal chain) raises at creation and names the frame floor.  The floor is inherited from the CRN geometry the engine's STFT used to be checked against, not FullSubNet's own
    (DESIGN.md 7): this test pins the UNCHANGED acceptance, so that lifting the floor is a decision with a test of its own."""
    from conftest import FSN_TINY
    from speech_enhancement_mi_amd.engine import FsnEngine
    cfg = FSN_TINY
    hop = cfg["sample_rate"] // 1000 * cfg["hop_length"]

    def make(seg):
        return FsnEngine(cfg["num_freqs"], cfg["num_mics"], cfg["fb_model_hidden_size"], cfg["sb_model_hidden_size"], cfg["num_layers"],
                         cfg["sb_num_neighbors"], cfg["fb_num_neighbors"], cfg["look_ahead"], cfg["sample_rate"], seg,
                         cfg["win_length"], cfg["hop_length"], cfg["n_fft"])
    with pytest.raises(RuntimeError, match=f"{frames} frames per segment: more than 16 frames"):
        make(hop * (frames - 1))
    make(hop * 16).close()   # 17 frames: accepted
