"""GPU tests of the fp16 pair format on the convolution / skip path (SE_F16_PAIR_CONV): xinP[i >= 1], decinP and decP as
two scaled fp16 planes, k_conv_p (all but encoder 0) and k_skip_p on three f16 MFMA terms, behind the extended range guard.  The
small plane-route configuration of test_gpu_f16_pair.py (channels [8, 8, 16, 32], hidden 64, 512-pt, SE_GEMM_SKINNY_ROWS=0; batches
of 17 and 40) and FULL512 at 4 streams; three segments, flag False then True.  SE_F16_PAIR_CONV=0 is the parent's state (the pair on
the bottleneck only), SE_F16_PAIR=0 the bf16 route everywhere."""
import numpy as np
import pytest

from conftest import FULL512, STUDENT400, TINY, rel_rms, spec_of
from engine_cases import SMALL as CFG, carried_state as _state, cuda as _cuda, make_engine, snapshot, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

L1, L2 = 6400, 4800  # three segments, then two more with the carried state
TAPS = ["feat", "enc0", "enc1", "enc2", "enc3", "gru", "dec0", "dec1", "dec2"]
SKIP_STREAM = {"SE_SKIP_MIN_BATCH": "1"}  # k_skip_p at every batch; without it batches below 96 take the two-launch kPOutBlend form


def _engine(cfg, env, monkeypatch, seed=4, precision=0, variant=0, sd=None):
    """An engine created under `env` (the knobs are read at creation; every engine here is on the plane GEMM route)."""
    return make_engine(cfg, monkeypatch, dict({"SE_GEMM_SKINNY_ROWS": "0"}, **env), seed=seed, precision=precision, variant=variant, sd=sd)


@pytest.fixture(scope="module")
def audio():
    return utterances(40, L1 + L2, seed=61)


def _snapshot(e, cfg, y):
    return snapshot(e, cfg, y, TAPS)


@pytest.mark.parametrize("name,cfg,batch,env", [("small17", CFG, 17, SKIP_STREAM), ("small40", CFG, 40, {}), ("full512", FULL512, 4, SKIP_STREAM),
                                                ("full512_two_launch", FULL512, 4, {})])
def test_default_against_the_other_routes(name, cfg, batch, env, audio, monkeypatch):
    """The default against SE_F16_PAIR_CONV=0 and against SE_F16_PAIR=0: outputs, taps and carried state within 2e-6, the project's
    bar between two fp32-accurate routes.  Not bit-equal to SE_F16_PAIR_CONV=0 (the route is on); the features and buf0 bit-equal to
    it, enc0 equal up to the storage format of encoder 0's output (encoder 0 reads the features, which keep their bf16 planes, and
    writes fp32)."""
    e_new = _engine(cfg, env, monkeypatch)
    e_par = _engine(cfg, dict(env, SE_F16_PAIR_CONV="0"), monkeypatch)
    e_old = _engine(cfg, dict(env, SE_F16_PAIR="0"), monkeypatch)
    differs = False
    for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
        x = _cuda(audio[:batch, :, lo:hi])
        snaps = [_snapshot(e, cfg, e.realtime_process(x, flag=flag).cpu().numpy()) for e in (e_new, e_par, e_old)]
        new, par, old = snaps
        assert np.isfinite(new["out"]).all() and np.abs(old["out"]).max() > 0
        differs |= not np.array_equal(new["out"], par["out"])
        for other, ref in (("SE_F16_PAIR_CONV=0", par), ("SE_F16_PAIR=0", old)):
            r = {k: rel_rms(new[k], ref[k]) for k in new}
            print(f"{name} flag {flag} vs {other}: " + "  ".join(f"{k} {v:.2e}" for k, v in r.items()))
            for k, v in r.items():
                assert v < 2e-6, (name, flag, other, k, v)
        # encoder 0 and the features did not change: the feature planes and their history have the same bits.  The tap enc0 is
        # xinP[1], encoder 0's normalised output AS STORED: bit-equal fp32 values, there in three bf16 planes (exact), here in the fp16
        # pair, which gives a value back to 2^-23 relative (2^-36 absolute) - element by element, that and nothing more
        assert np.array_equal(new["feat"], par["feat"]) and np.array_equal(new["buf0"], par["buf0"]), "the features changed"
        d, ref0 = np.abs(new["enc0"].astype(np.float64) - par["enc0"]), np.abs(par["enc0"].astype(np.float64))
        assert np.all(d <= np.maximum(ref0 * 2.0 ** -23, 2.0 ** -36)), "encoder 0 changed by more than the storage of its output"
        assert not np.array_equal(new["enc2"], par["enc2"]) or not np.array_equal(new["dec0"], par["dec0"])
    assert differs, "the default gives the bits of SE_F16_PAIR_CONV=0: the convolution path is not on the fp16 pair"


@pytest.mark.parametrize("env", [{"SE_DEC_PAIR": "0"}, {"SE_DEC_PAIR": "1"}, {"SE_PIPELINE": "0"}, {"SE_IO_FUSE": "0"},
                                 {"SE_PIPELINE": "0", "SE_SKIP_MIN_BATCH": "1"}], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_route_variants_same_bar(env, audio, monkeypatch):
    """One launch per decoder parity or both in one, one stream, the unfused STFT / iSTFT kernels; the skip gate as two k_conv_p
    launches (default at these batches) and as k_skip_p: the default within 2e-6 of SE_F16_PAIR=0 under the same knob."""
    for batch in (17, 40):
        e_new, e_old = _engine(CFG, env, monkeypatch), _engine(CFG, dict(env, SE_F16_PAIR="0"), monkeypatch)
        for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
            x = _cuda(audio[:batch, :, lo:hi])
            new = _snapshot(e_new, CFG, e_new.realtime_process(x, flag=flag).cpu().numpy())
            old = _snapshot(e_old, CFG, e_old.realtime_process(x, flag=flag).cpu().numpy())
            r = {k: rel_rms(new[k], old[k]) for k in new}
            print(f"{env} batch {batch} flag {flag}: " + "  ".join(f"{k} {v:.2e}" for k, v in r.items()))
            assert np.abs(old["out"]).max() > 0
            for k, v in r.items():
                assert v < 2e-6, (env, batch, flag, k, v)


@pytest.mark.parametrize("batch,env", [(17, SKIP_STREAM), (40, {})])
def test_forward_stages_against_oracle(batch, env, audio, monkeypatch):
    """Three consecutive frames through forward() with the state carried (test_gpu_parity.test_forward_stages_vs_oracle): output
    within 1e-4, every tap and the carried state within 2e-5 of the oracle."""
    from oracle import crn_oracle as orc
    e = _engine(CFG, env, monkeypatch)
    o = orc.CrnOracle(**CFG)
    o.load_state_dict(synth.make_state_dict(spec_of(CFG), seed=4))
    e.reset(batch)
    o.reset(batch)
    F = CFG["num_freqs"]
    for n in range(3):
        seg = np.ascontiguousarray(audio[:batch, :, n * 1600:n * 1600 + 3200])
        x = o.stft(seg.reshape(-1, 3200)).reshape(batch, 3, F, 21, 2)
        yo = o.forward(x)
        ye = e.forward(_cuda(x)).cpu().numpy()
        r = {"out": rel_rms(ye, yo), **{t: rel_rms(e.read_tap(t), o.tap(t)) for t in TAPS}}
        print(f"batch {batch} frame {n}: " + "  ".join(f"{k} {v:.2e}" for k, v in r.items()))
        assert r.pop("out") < 1e-4
        for k, v in r.items():
            assert v < 2e-5, (n, k, v)
    for k, v in _state(e, CFG).items():
        assert rel_rms(v, o.state(k)) < 2e-5, k


def test_full512_against_oracle(audio, monkeypatch):
    from oracle import crn_oracle as orc
    e = _engine(FULL512, SKIP_STREAM, monkeypatch)
    o = orc.CrnOracle(**FULL512)
    o.load_state_dict(synth.make_state_dict(spec_of(FULL512), seed=4))
    x = np.ascontiguousarray(audio[:4, :, :9600])
    r = rel_rms(e.realtime_process(_cuda(x)).cpu().numpy(), o.realtime_process(x))
    print(f"FULL512, 4 x 9600 samples vs oracle: {r:.2e}")
    assert r < 1e-4


def test_ragged_batch_matches_streams_alone(audio, monkeypatch):
    """Per-stream lengths (test_gpu_f16_pair.test_pair_route_ragged_batch_matches_streams_alone): the state rows of the two-plane
    rings are saved and restored per stream; every stream stays within 2e-6 of its run alone."""
    e = _engine(CFG, SKIP_STREAM, monkeypatch)
    L = L1 + L2
    lens = [L - 1600 * (b % 4) - 37 * (b % 3) for b in range(40)]
    y = e.realtime_process(_cuda(audio[:, :, :L]), lengths=lens).cpu().numpy()
    e1 = _engine(CFG, SKIP_STREAM, monkeypatch)
    for b in (0, 1, 2, 3, 17, 38, 39):
        alone = e1.realtime_process(_cuda(audio[b:b + 1, :, :lens[b]])).cpu().numpy()
        r = rel_rms(y[b, :lens[b]], alone[0])
        print(f"stream {b}: {r:.2e}")
        assert r < 2e-6, b
        assert np.all(y[b, lens[b]:] == 0), b


@pytest.mark.parametrize("batch", [17, 40])
def test_state_round_trip_is_bit_exact(batch, audio, monkeypatch):
    """export_state of every buf{i} and h after call 1 -> import_state on a fresh engine: call 2 equals the continuing engine's call 2
    bit for bit (split2h(join2h(.)) is the identity on stored pairs: tests/f16_pair_conv_check.cpp asserts it on the host)."""
    e = _engine(CFG, SKIP_STREAM, monkeypatch)
    e.realtime_process(_cuda(audio[:batch, :, :L1]))
    st = _state(e, CFG)
    fresh = _engine(CFG, SKIP_STREAM, monkeypatch)
    fresh.reset(batch)
    for k, v in st.items():
        fresh.import_state(k, v)
    for k, v in _state(fresh, CFG).items():
        assert np.array_equal(v, st[k]), k
    x2 = _cuda(audio[:batch, :, L1:L1 + L2])
    y_cont, y_fresh = e.realtime_process(x2, flag=True).cpu().numpy(), fresh.realtime_process(x2, flag=True).cpu().numpy()
    assert np.abs(y_cont).max() > 0
    assert np.array_equal(y_cont, y_fresh)


def test_loud_input(audio, monkeypatch):
    """Input scaled by 3e4: the features keep their bf16 planes, every pair-format buffer sits behind a norm or the skip gate's
    convex combination - finite output, within 2e-6 of the bf16 route."""
    e_new, e_old = _engine(CFG, SKIP_STREAM, monkeypatch), _engine(CFG, dict(SKIP_STREAM, SE_F16_PAIR="0"), monkeypatch)
    x = _cuda(3e4 * audio[:17, :, :L1])
    y_new, y_old = e_new.realtime_process(x).cpu().numpy(), e_old.realtime_process(x).cpu().numpy()
    assert np.isfinite(y_new).all() and np.abs(y_new).max() > 0
    r = rel_rms(y_new, y_old)
    print(f"input x 3e4: {r:.2e}")
    assert r < 2e-6


def test_skip_bound_guard_keeps_the_bf16_route(audio, monkeypatch):
    """FULL512 with one row of deconvlist.0.residual.weight at 15.0: every weight stays below 16 and every norm is unchanged, but the
    skip output's bound is 64 x 15 = 960 times the bound of the encoder norm behind `res` (about 253) - beyond 6e4, so the whole
    engine runs the bf16 route: the bits of SE_F16_PAIR=0."""
    sd = {k: np.array(v, dtype=np.float32, copy=True) for k, v in synth.make_state_dict(spec_of(FULL512), seed=4).items()}
    w = sd["deconvlist.0.residual.weight"]
    w.reshape(w.shape[0], -1)[3, :] = 15.0
    e_new, e_old = _engine(FULL512, {}, monkeypatch, sd=sd), _engine(FULL512, {"SE_F16_PAIR": "0"}, monkeypatch, sd=sd)
    x = _cuda(audio[:4, :, :L1])
    y_new, y_old = e_new.realtime_process(x).cpu().numpy(), e_old.realtime_process(x).cpu().numpy()
    assert np.isfinite(y_old).all() and np.abs(y_old).max() > 0
    assert np.array_equal(y_new, y_old)


@pytest.mark.parametrize("case", ["precision1", "precision2", "crn_elu", "student"])
def test_knob_leaves_ineligible_routes_alone(case, audio, monkeypatch):
    """fp16 operands, bf16x3, CRN_ELU and the student are not eligible: SE_F16_PAIR_CONV either way, the same bits."""
    cfg, precision, variant = {"precision1": (CFG, 1, 0), "precision2": (CFG, 2, 0), "crn_elu": (TINY, 0, 1), "student": (STUDENT400, 0, 2)}[case]
    x = _cuda(audio[:17 if cfg is CFG else 3, :, :L1])
    ys = []
    for env in ({"SE_F16_PAIR_CONV": "1"}, {"SE_F16_PAIR_CONV": "0"}):
        ys.append(_engine(cfg, env, monkeypatch, seed=0, precision=precision, variant=variant).realtime_process(x).cpu().numpy())
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])


@pytest.mark.parametrize("direction", ["pair_to_bf16", "bf16_to_pair"])
def test_weight_load_that_flips_the_format_of_a_running_batch(direction, audio, monkeypatch):
    """A running batch gets a checkpoint on the other side of the range guard (one convolution weight of 40 fails it): the format of
    the plane buffers flips between two calls, the conv history of the current ring slot is re-written in the new format, the tilings
    are selected again and the statistics slabs follow them.  72 streams of the small configuration: the last decoder block runs 11
    workgroups per stream on bf16 planes and 6 on the pair, so the slab of one format is too small for the other.  Call 2 (flag=True)
    has the bits of a fresh engine that loaded the second checkpoint and imported the state, and stays within 2e-6 of an engine that
    ran the bf16 route all along."""
    B = 72
    good = synth.make_state_dict(spec_of(CFG), seed=4)
    bad = {k: np.array(v, dtype=np.float32, copy=True) for k, v in good.items()}
    for k in ("convlist.2.conv.weight", "convlist.2.net.0.weight"):  # (one tensor under the reference's two names)
        if k in bad:
            bad[k].reshape(-1)[5] = 40.0
    first, second = (good, bad) if direction == "pair_to_bf16" else (bad, good)
    wide = np.concatenate([audio, 0.7 * audio[:B - 40]], axis=0)
    x1, x2 = _cuda(wide[:, :, :L1]), _cuda(wide[:, :, L1:L1 + L2])
    e_new, e_old = _engine(CFG, {}, monkeypatch, sd=first), _engine(CFG, {"SE_F16_PAIR": "0"}, monkeypatch, sd=first)
    for e in (e_new, e_old):
        e.realtime_process(x1)
        e.load_state_dict(second)
    st = _state(e_new, CFG)  # (read in the format the ring still holds: the flip happens at the next call)
    fresh = _engine(CFG, {}, monkeypatch, sd=second)
    fresh.reset(B)
    for k, v in st.items():
        fresh.import_state(k, v)
    y_new, y_old, y_fresh = (e.realtime_process(x2, flag=True).cpu().numpy() for e in (e_new, e_old, fresh))
    assert np.isfinite(y_old).all() and np.abs(y_old).max() > 0
    r = rel_rms(y_new, y_old)
    print(f"{direction}: against the bf16 route {r:.2e}")
    assert r < 2e-6
    assert np.array_equal(y_new, y_fresh), "the flipped engine and a fresh engine with the imported state differ"
    y3_new, y3_fresh = (e.realtime_process(x1, flag=True).cpu().numpy() for e in (e_new, fresh))  # the state both left behind
    assert np.array_equal(y3_new, y3_fresh)
