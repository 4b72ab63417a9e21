"""fsn_realtime_process_chains on the GPU: B FullSubNet chunk chains in one call, each stream with its own length, its own flag and its
own CumLayerNorm step counters, each leaving exactly the state it would carry alone; fsn_reset_stream and state hand-over
(DESIGN.md 6 "Batched chunk chains in the FullSubNet engine")."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import FSN_FULL, FSN_TINY, ROOT, rel_rms
from engine_cases import cuda as _cuda, make_fsn_engine as _engine
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd.engine import chain_geometry

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's parity bar against the reference (tests/test_gpu_parity.py)
BAR_ALONE = 2e-6    # batch against each stream alone: BAR_ALONE of tests/test_gpu_engine_chains.py
K = FSN_FULL["segment_length"]
STATE_NAMES = ("fh", "fc", "sh", "sc", "mean_fb", "mean_sb", "step_fb", "step_sb")
SE_ERR_ARG, SE_ERR_KEY, SE_ERR_STATE = -1, -2, -4

# the cases of tests/golden/make_golden_fsn_chain.py
SEED, TOTAL = 21, 12800
CALLS = (((False, False, False), (8000, 5200, 3400)), ((True, False, True), (4800, 7000, 3300)))


def _batches(calls, seed, pad):
    """one [B, M, Lmax] batch per call (lens, flags), `pad` beyond every stream's own length: the engine must not read it"""
    xs = []
    for c, (lens, _) in enumerate(calls):
        mix, _ = synth.synth_utterances(len(lens), max(lens), 3, seed=seed + c)
        for b, l in enumerate(lens):
            mix[b, :, l:] = pad
        xs.append(mix)
    return xs


def _stream_state(e, cfg, B, b):
    """every state name of stream b of a batch of B, flat"""
    NL, out = cfg["num_layers"], {}
    for n in STATE_NAMES:
        a = e.export_state(n)
        out[n] = a.reshape(NL, B, -1)[:, b].reshape(-1).copy() if n in ("fh", "fc", "sh", "sc") else a.reshape(B)[b:b + 1].copy()
    return out


def _run_batch(cfg, calls, xs, precision=0, seed=0, states=True):
    e = _engine(cfg, precision=precision, seed=seed)
    B = len(calls[0][0])
    ys, sts = [], []
    for c, (lens, flags) in enumerate(calls):
        ys.append(e.realtime_process(_cuda(xs[c]), flag=[bool(f) for f in flags], lengths=lens).cpu().numpy())
        sts.append([_stream_state(e, cfg, B, b) for b in range(B)] if states else None)
    return ys, sts


def _run_alone(cfg, calls, xs, streams, precision=0, seed=0, states=True):
    """every listed stream's chain by itself on one batch-1 engine -> ys[c][b], sts[c][b][name]"""
    e1 = _engine(cfg, precision=precision, seed=seed)
    ys, sts = [dict() for _ in calls], [dict() for _ in calls]
    for b in streams:
        for c, (lens, flags) in enumerate(calls):
            ys[c][b] = e1.realtime_process(_cuda(xs[c][b:b + 1, :, :lens[b]]), flag=bool(flags[b])).cpu().numpy()[0]
            if states:
                sts[c][b] = _stream_state(e1, cfg, 1, 0)
    return ys, sts


def _check(calls, ys, sts, ys1, sts1, streams, bar, what):
    """outputs (and states, where given) of the batch against every stream alone; returns the largest error seen"""
    worst = 0.0
    for c, (lens, _) in enumerate(calls):
        for b in streams:
            l = lens[b]
            err = rel_rms(ys[c][b, :l], ys1[c][b])
            worst = max(worst, err)
            print(f"{what} call {c + 1} stream {b} (length {l}): output rel rms {err:.3e}")
            assert err <= bar, (what, c, b, l, err)
            assert np.all(ys[c][b, l:] == 0.0), (what, c, b)
            if sts is None or sts[c] is None:
                continue
            for n in STATE_NAMES:
                got, ref = sts[c][b][n], sts1[c][b][n]
                if n.startswith("step"):
                    assert np.array_equal(got, ref), (what, c, b, n, got, ref)
                    continue
                if not np.any(ref):
                    assert np.max(np.abs(got)) <= 1e-6, (what, c, b, n)
                    continue
                err = rel_rms(got, ref)
                worst = max(worst, err)
                if err > 0:
                    print(f"{what} call {c + 1} stream {b}: state {n} rel rms {err:.3e}")
                assert err <= bar, (what, c, b, n, err)
    print(f"{what}: largest error {worst:.3e}")
    return worst


# ---- 1. the reference fixture ------------------------------------------------------------------------------------------------
def _fixture_batch(call):
    mix = synth.synth_utterances(3, TOTAL, FSN_TINY["num_mics"], seed=SEED)[0]
    lens = CALLS[call][1]
    x = np.full((3, mix.shape[1], max(lens)), 3.0, np.float32)
    for b, L in enumerate(lens):
        lo = 0 if call == 0 else CALLS[0][1][b]
        x[b, :, :L] = mix[b, :, lo:lo + L]
    return x


@pytest.mark.parametrize("pipeline", ["1", "0"], ids=["pipelined", "serial"])
def test_chains_match_the_reference_fixture(pipeline, monkeypatch):
    """The two calls of make_golden_fsn_chain.py through FsnEngine.realtime_process with per-stream flags: every utterance equals what
    the genuine reference gives for it ALONE (fsn_chain_golden.npz), zeros beyond its length.  Call 1 runs 8 / 6 / 6 windows: utterances
    1 and 2 end early (a missing save fails call 2 of utterance 2); call 2 mixes continue / reset / continue (collapsed flags or a
    shared step counter fail)."""
    monkeypatch.setenv("SE_FSN_PIPELINE", pipeline)
    g = np.load(os.path.join(ROOT, "tests", "golden", "fsn_chain_golden.npz"))
    e = _engine(FSN_TINY)
    assert chain_geometry(CALLS[0][1], CALLS[0][0], K)["Nb"] == [8, 6, 6]
    for c, (flags, lens) in enumerate(CALLS):
        y = e.realtime_process(_cuda(_fixture_batch(c)), flag=list(flags), lengths=list(lens)).cpu().numpy()
        for b, l in enumerate(lens):
            err = rel_rms(y[b, :l], g[f"call{c + 1}_utt{b}"])
            print(f"fixture pipeline={pipeline} call {c + 1} utt {b}: rel rms {err:.3e}")
            assert err < TOL, (c, b, err)
            assert np.all(y[b, l:] == 0.0), (c, b)


# ---- 2. each stream equals its own chain alone ----------------------------------------------------------------------------------
def _case2_calls():
    """batch 4, three calls, lengths between 0.3 s and 1.5 s (fixed seed); per call one stream at 0.3 s and another at 1.5 s"""
    rng = np.random.default_rng(11)
    calls = []
    for c, flags in enumerate(([0, 0, 0, 0], [1, 1, 0, 1], [1, 1, 1, 1])):
        lens = [int(v) for v in rng.integers(4800, 24001, 4)]
        lens[c % 4], lens[(c + 2) % 4] = 4800, 24000
        calls.append((lens, flags))
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def _case2(precision):
    calls = _case2_calls()
    xs = _batches(calls, 60, 7.0)
    ys, sts = _run_batch(FSN_FULL, calls, xs, precision)
    ys1, sts1 = _run_alone(FSN_FULL, calls, xs, range(4), precision)
    return calls, ys, sts, ys1, sts1


@pytest.mark.parametrize("precision", [0, 2], ids=["fp32", "bf16x3"])
def test_each_stream_equals_its_own_chain_alone(precision):
    """FSN_FULL, 4 streams, three calls, 7.0 beyond every length; one engine at batch 4 against one engine at batch 1 that runs every
    stream's chain by itself.  After EVERY call: the output and all eight state names (LSTM states of both models, both running means,
    both step counters) per stream.  In every call some stream ends at least 5 windows before the longest one, so its state must have
    been saved when it ended; call 2 resets stream 2 among continuing streams."""
    calls, ys, sts, ys1, sts1 = _case2(precision)
    for lens, flags in calls:
        nb = chain_geometry(lens, flags, K)["Nb"]
        assert max(nb) - min(nb) >= 5, nb
    assert calls[1][1] == [1, 1, 0, 1]
    _check(calls, ys, sts, ys1, sts1, range(4), BAR_ALONE, f"case 2 precision {precision}")


# ---- 3. per-stream step counters, cap included --------------------------------------------------------------------------------------
def test_step_counters_are_per_stream():
    """FSN_TINY, batch 2, two calls of 70 000 samples (46 windows each): stream 0 continues and crosses the cap of 80
    (fullsubnet.py:197-198), stream 1 is reset in call 2 and stays below it, so in call 2 the two streams update their running means
    with different alpha = step / (step + 1) in every window.  One counter for the whole batch cannot give both."""
    calls = (([70000, 70000], [0, 0]), ([70000, 70000], [1, 0]))
    xs = _batches(calls, 90, 0.0)
    ys, sts = _run_batch(FSN_TINY, calls, xs)
    ys1, sts1 = _run_alone(FSN_TINY, calls, xs, range(2))
    _check(calls, ys, sts, ys1, sts1, range(2), BAR_ALONE, "case 3")
    n0 = [chain_geometry(l, f, K)["Nb"] for l, f in calls]
    assert n0[0][0] + n0[1][0] > 80 and n0[1][1] < 80
    for n in ("step_fb", "step_sb"):
        got = [float(sts[1][b][n][0]) for b in range(2)]
        assert got == [80.0, float(n0[1][1])], (n, got)


# ---- 4. compaction across the LSTM-tile threshold -----------------------------------------------------------------------------------
FSN_64 = dict(FSN_FULL, fb_model_hidden_size=64, sb_model_hidden_size=64)


def _case4_calls():
    B = 44
    rng = np.random.default_rng(17)
    l1 = [int(v) for v in rng.integers(1600, 6401, B)]
    for b in (3, 17, 30, 41):   # four long streams: the active prefix is 4 streams for the last windows
        l1[b] = 14400 + 100 * b
    l2 = [int(v) for v in rng.integers(1600, 8001, B)]
    f2 = [0 if b % 4 == 1 else 1 for b in range(B)]
    return ((l1, [0] * B), (l2, f2))


def test_compaction_across_the_lstm_tile_threshold():
    """44 streams x 201 sub-band rows = 8 844 >= 8 192 rows with H = 64: the carried batch takes the 256-row LSTM tile.  The shim sorts
    the fresh batch by window count, and the prefix of running streams falls from 44 to 4 (below the 41 streams the tile threshold
    asks for) while 5 windows remain.  Call 2 continues the carried, unsorted batch with every fourth stream reset.  Every stream of
    both calls against its chain alone; the whole sequence twice, bit for bit."""
    calls = _case4_calls()
    nb = chain_geometry(calls[0][0], calls[0][1], K)["Nb"]
    running = [sum(1 for v in nb if v > n) for n in range(max(nb))]
    assert running[0] == 44 and sum(1 for r in running if r < 41) >= 5 and sorted(nb, reverse=True) != nb, running
    xs = _batches(calls, 70, -3.0)
    ys, _ = _run_batch(FSN_64, calls, xs, states=False)
    ys1, _ = _run_alone(FSN_64, calls, xs, range(44), states=False)
    _check(calls, ys, None, ys1, None, range(44), BAR_ALONE, "case 4")
    ys_b, _ = _run_batch(FSN_64, calls, xs, states=False)
    for a, b in zip(ys, ys_b):
        assert np.array_equal(a, b)


# ---- 5. a uniform batch is fsn_realtime_process ---------------------------------------------------------------------------------------
def _uniform_is_plain(ea, eb):
    mix, _ = synth.synth_utterances(3, 2 * 9000, 3, seed=81)
    for c, flag in enumerate((False, True)):
        x = _cuda(mix[:, :, c * 9000:(c + 1) * 9000])
        ya = ea.realtime_process_chains(x, [flag] * 3, [9000] * 3)
        yb = eb.realtime_process(x, flag=flag)
        assert torch.equal(ya, yb), flag
        for n in STATE_NAMES:
            assert np.array_equal(ea.export_state(n), eb.export_state(n)), (flag, n)


def test_uniform_batch_is_fsn_realtime_process():
    _uniform_is_plain(_engine(FSN_TINY), _engine(FSN_TINY))


# ---- 6. hand-over ----------------------------------------------------------------------------------------------------------------
def test_state_hand_over_between_engines():
    """Stream 1 of engine A (batch 3, sorted slots) is exported after call 1 and imported into slot 0 of a batch-1 engine B; its call 2
    on B equals its call 2 on A."""
    calls = (([6000, 11000, 8000], [0, 0, 0]), ([5000, 7000, 4000], [1, 1, 1]))
    xs = _batches(calls, 40, 5.0)
    A, Bn = _engine(FSN_TINY), _engine(FSN_TINY)
    A.realtime_process(_cuda(xs[0]), flag=[False] * 3, lengths=calls[0][0])
    assert A._order is not None   # the fresh batch was sorted: export speaks the caller's rows all the same
    Bn.reset(1)
    for n in STATE_NAMES:
        a = A.export_state(n)
        Bn.import_state(n, a.reshape(FSN_TINY["num_layers"], 3, -1)[:, 1] if n in ("fh", "fc", "sh", "sc") else a.reshape(3)[1:2])
    ya = A.realtime_process(_cuda(xs[1]), flag=[True] * 3, lengths=calls[1][0]).cpu().numpy()
    l = calls[1][0][1]
    yb = Bn.realtime_process(_cuda(xs[1][1:2, :, :l]), flag=True).cpu().numpy()
    err = rel_rms(yb[0], ya[1, :l])
    print(f"hand-over: continuation on B against A rel rms {err:.3e}")
    assert err <= BAR_ALONE, err
    with pytest.raises(RuntimeError):
        A.reset_stream(3)


def test_reset_stream_then_flagged_call_is_a_chains_reset():
    """reset_stream(i) followed by a call with every flag set, in which caller i supplies the K/2 zeros of a first chunk itself and
    strips them again (what realtime_process(flag=False) does, fullsubnet.py:905-907, 956-957), equals a chains call with flags[i] = 0."""
    i, P = 1, K // 2
    calls = (([9000, 5000, 7000], [0, 0, 0]), ([4000, 6000, 5000], [1, 0, 1]))
    xs = _batches(calls, 50, 0.0)
    X, Y = _engine(FSN_TINY), _engine(FSN_TINY)
    for e in (X, Y):
        e.realtime_process(_cuda(xs[0]), flag=[False] * 3, lengths=calls[0][0])
    yy = Y.realtime_process(_cuda(xs[1]), flag=[True, False, True], lengths=calls[1][0]).cpu().numpy()
    X.reset_stream(i)
    lens = list(calls[1][0])
    lens[i] += P
    x2 = np.zeros((3, 3, max(lens)), np.float32)
    for b in range(3):
        lo = P if b == i else 0
        x2[b, :, lo:lo + calls[1][0][b]] = xs[1][b, :, :calls[1][0][b]]
    yx = X.realtime_process(_cuda(x2), flag=[True] * 3, lengths=lens).cpu().numpy()
    for b in range(3):
        l, lo = calls[1][0][b], (P if b == i else 0)
        err = rel_rms(yx[b, lo:lo + l], yy[b, :l])
        print(f"reset_stream: stream {b} rel rms {err:.3e}")
        assert err <= BAR_ALONE, (b, err)
    for n in STATE_NAMES:
        a, b_ = X.export_state(n), Y.export_state(n)
        assert rel_rms(a, b_) <= BAR_ALONE, n


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_chain_errors_leave_the_engine_usable():
    e = _engine(FSN_TINY)
    x = _cuda(_fixture_batch(0))
    lens = list(CALLS[0][1])
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_STATE}:"):     # nothing is carried yet
        e.realtime_process(x, flag=[True, False, False], lengths=lens)
    e.realtime_process(x, flag=[False] * 3, lengths=lens)
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_STATE}:.*carried state holds 3 streams"):
        e.realtime_process(x[:2].contiguous(), flag=[True, False], lengths=lens[:2])
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_ARG}:.*outside"):
        e.realtime_process(x, flag=[True, False, True], lengths=[lens[0], 0, lens[2]])
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_ARG}:.*outside"):
        e.realtime_process(x, flag=[True, False, True], lengths=[lens[0], x.shape[2] + 1, lens[2]])
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_KEY}:"):
        e.export_state("nope")
    with pytest.raises(RuntimeError, match=f"error {SE_ERR_KEY}:"):
        e.import_state("nope", np.zeros(3, np.float32))
    # none of the refused calls touched the carried state: call 2 of the fixture still comes out right ...
    g = np.load(os.path.join(ROOT, "tests", "golden", "fsn_chain_golden.npz"))
    flags2, lens2 = CALLS[1]
    y2 = e.realtime_process(_cuda(_fixture_batch(1)), flag=list(flags2), lengths=list(lens2)).cpu().numpy()
    for b, l in enumerate(lens2):
        assert rel_rms(y2[b, :l], g[f"call2_utt{b}"]) < TOL, b
    # ... and the engine passes the uniform-batch test again
    _uniform_is_plain(e, _engine(FSN_TINY))
