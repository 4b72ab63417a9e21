"""GPU tests of the fp16 pair operand format on the bottleneck (csrc/split_f16pair.h, SE_F16_PAIR): gruinP / seqP as two
scaled fp16 planes, k_gemm_p and the GRU step on three f16 MFMA terms.  The small plane-route configuration of test_gpu_gru_split.py
(D = 544, hidden 64, SE_GEMM_SKINNY_ROWS=0, SE_SKIP_MIN_BATCH=1; batches of 17 and 40: a partial 32-row tile, two unit groups, both
step kernels) and FULL512 at 4 streams; three segments, flag False then True."""
import numpy as np
import pytest

from conftest import FSN_TINY, FULL512, STUDENT400, TINY, rel_rms, spec_of
from engine_cases import SMALL as CFG, cuda as _cuda, carried_state, make_engine, make_fsn_engine, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

L1, L2 = 6400, 4800  # three segments, then two more with the carried state
TAPS = ["gru", "dec0", "dec2", "enc0", "enc1", "enc2", "enc3"]


def _engine(cfg, env, monkeypatch, seed=4, precision=0, variant=0, sd=None):
    """An engine created under `env` (the knobs are read at creation; every engine here is on the plane GEMM route)."""
    return make_engine(cfg, monkeypatch, dict({"SE_GEMM_SKINNY_ROWS": "0", "SE_SKIP_MIN_BATCH": "1"}, **env), seed=seed, precision=precision,
                       variant=variant, sd=sd)


@pytest.fixture(scope="module")
def audio():
    return utterances(40, L1 + L2, seed=61)


def _state(e, cfg):
    return list(carried_state(e, cfg).values())  # h, buf0, buf1, ...


@pytest.mark.parametrize("name,cfg,batch", [("small17", CFG, 17), ("small40", CFG, 40), ("full512", FULL512, 4)])
def test_pair_route_against_bf16_route(name, cfg, batch, audio, monkeypatch):
    """SE_F16_PAIR=0 (six bf16 terms) against the default: outputs, taps and carried state within 2e-6, the project's bar between two
    fp32-accurate routes - and not bit-equal, which shows that the route is on."""
    e_new, e_old = _engine(cfg, {}, monkeypatch), _engine(cfg, {"SE_F16_PAIR": "0"}, monkeypatch)
    differs = False
    for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
        x = _cuda(audio[:batch, :, lo:hi])
        y_new, y_old = e_new.realtime_process(x, flag=flag).cpu().numpy(), e_old.realtime_process(x, flag=flag).cpu().numpy()
        assert np.isfinite(y_new).all() and np.abs(y_old).max() > 0
        differs |= not np.array_equal(y_new, y_old)
        r = {"out": rel_rms(y_new, y_old)}
        for tap in TAPS:
            r[tap] = rel_rms(e_new.read_tap(tap), e_old.read_tap(tap))
        for i, (a, b) in enumerate(zip(_state(e_new, cfg), _state(e_old, cfg))):
            r["h" if i == 0 else f"buf{i - 1}"] = rel_rms(a, b)
        print(f"{name} flag {flag}: " + "  ".join(f"{k} {v:.2e}" for k, v in r.items()))
        for k, v in r.items():
            assert v < 2e-6, (name, flag, k, v)
    assert differs, "the default route gives the bits of SE_F16_PAIR=0: the fp16 pair format is not on"


@pytest.mark.parametrize("batch", [17, 40])
def test_pair_route_forward_against_oracle(batch, audio, monkeypatch):
    """Three consecutive frames through forward() with the state carried (test_gpu_parity.test_forward_stages_vs_oracle): output
    within 1e-4, the decoder-input tap and h within 2e-5 of the oracle."""
    from oracle import crn_oracle as orc
    e = _engine(CFG, {}, monkeypatch)
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
        r_out, r_gru, r_enc = rel_rms(ye, yo), rel_rms(e.read_tap("gru"), o.tap("gru")), rel_rms(e.read_tap("enc3"), o.tap("enc3"))
        print(f"batch {batch} frame {n}: out {r_out:.2e}  gru tap {r_gru:.2e}  enc3 tap {r_enc:.2e}")
        assert r_out < 1e-4 and r_gru < 2e-5 and r_enc < 2e-5, (n, r_out, r_gru, r_enc)
    assert rel_rms(e.export_state("h"), o.state("h")) < 2e-5


def test_pair_route_full512_against_oracle(audio, monkeypatch):
    from oracle import crn_oracle as orc
    e = _engine(FULL512, {}, monkeypatch)
    o = orc.CrnOracle(**FULL512)
    o.load_state_dict(synth.make_state_dict(spec_of(FULL512), seed=4))
    x = np.ascontiguousarray(audio[:4, :, :9600])
    r = rel_rms(e.realtime_process(_cuda(x)).cpu().numpy(), o.realtime_process(x))
    print(f"FULL512, 4 x 9600 samples vs oracle: {r:.2e}")
    assert r < 1e-4


def test_pair_route_ragged_batch_matches_streams_alone(audio, monkeypatch):
    """Per-stream lengths: the active rows shrink below one 32-row tile as the short streams end; every stream stays within 2e-6 of its
    run alone (a batch of one: the <= 16-stream step kernel writes the pair planes there)."""
    e = _engine(CFG, {}, monkeypatch)
    L = L1 + L2
    lens = [L - 1600 * (b % 4) - 37 * (b % 3) for b in range(40)]  # 40, 30, 20, 10 rows active over the last segments
    y = e.realtime_process(_cuda(audio[:, :, :L]), lengths=lens).cpu().numpy()
    e1 = _engine(CFG, {}, monkeypatch)
    for b in (0, 1, 2, 3, 17, 38, 39):
        alone = e1.realtime_process(_cuda(audio[b:b + 1, :, :lens[b]])).cpu().numpy()
        r = rel_rms(y[b, :lens[b]], alone[0])
        print(f"stream {b}: {r:.2e}")
        assert r < 2e-6, b
        assert np.all(y[b, lens[b]:] == 0), b


@pytest.mark.parametrize("batch", [17, 40])
def test_pair_route_pipelined_against_serial(batch, audio, monkeypatch):
    e_pip, e_ser = _engine(CFG, {}, monkeypatch), _engine(CFG, {"SE_PIPELINE": "0"}, monkeypatch)
    for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
        x = _cuda(audio[:batch, :, lo:hi])
        r = rel_rms(e_pip.realtime_process(x, flag=flag).cpu().numpy(), e_ser.realtime_process(x, flag=flag).cpu().numpy())
        print(f"batch {batch} flag {flag}: pipelined vs SE_PIPELINE=0 {r:.2e}")
        assert r < 2e-6


def test_pair_route_loud_input(audio, monkeypatch):
    """Input scaled by 3e4: the features (whose magnitude channel follows the input level) stay on bf16 planes, every pair-format
    buffer sits behind a norm - finite output, within 2e-6 of the bf16 route."""
    e_new, e_old = _engine(CFG, {}, monkeypatch), _engine(CFG, {"SE_F16_PAIR": "0"}, monkeypatch)
    x = _cuda(3e4 * audio[:17, :, :L1])
    y_new, y_old = e_new.realtime_process(x).cpu().numpy(), e_old.realtime_process(x).cpu().numpy()
    assert np.isfinite(y_new).all() and np.abs(y_new).max() > 0
    r = rel_rms(y_new, y_old)
    print(f"input x 3e4: {r:.2e}")
    assert r < 2e-6


@pytest.mark.parametrize("case", ["norm_gamma_400", "conv_weight_40"])
def test_range_guard_keeps_the_bf16_route(case, audio, monkeypatch):
    """A checkpoint whose activation bound or weight range does not fit fp16 runs the bf16 route: the bits of SE_F16_PAIR=0.
    FULL512: the first encoder norm covers 16 x 21 x 129 elements per stream, so gamma = 400 bounds its output by 400 sqrt(43344) = 8.3e4
    (in the small configuration no norm is wide enough for gamma = 400 to pass 6e4)."""
    cfg = FULL512
    sd = {k: np.array(v, dtype=np.float32, copy=True) for k, v in synth.make_state_dict(spec_of(cfg), seed=4).items()}
    if case == "norm_gamma_400":
        sd["convlist.0.norm.weight"].reshape(-1)[1] = 400.0
    else:
        for k in ("convlist.2.conv.weight", "convlist.2.net.0.weight"):  # (one tensor under the reference's two names)
            if k in sd:
                sd[k].reshape(-1)[5] = 40.0
    e_new, e_old = _engine(cfg, {}, monkeypatch, sd=sd), _engine(cfg, {"SE_F16_PAIR": "0"}, monkeypatch, sd=sd)
    x = _cuda(audio[:4, :, :L1])
    y_new, y_old = e_new.realtime_process(x).cpu().numpy(), e_old.realtime_process(x).cpu().numpy()
    assert np.isfinite(y_old).all() and np.abs(y_old).max() > 0
    assert np.array_equal(y_new, y_old)


@pytest.mark.parametrize("case", ["precision1", "precision2", "crn_elu", "student"])
def test_knob_leaves_other_routes_alone(case, audio, monkeypatch):
    """fp16 operands, bf16x3, CRN_ELU and the student are not eligible: SE_F16_PAIR either way, the same bits."""
    cfg, precision, variant = {"precision1": (CFG, 1, 0), "precision2": (CFG, 2, 0), "crn_elu": (TINY, 0, 1), "student": (STUDENT400, 0, 2)}[case]
    x = _cuda(audio[:17 if cfg is CFG else 3, :, :L1])
    ys = []
    for env in ({"SE_F16_PAIR": "1"}, {"SE_F16_PAIR": "0"}):
        ys.append(_engine(cfg, env, monkeypatch, seed=0, precision=precision, variant=variant).realtime_process(x).cpu().numpy())
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])


def test_knob_leaves_fullsubnet_alone(audio, monkeypatch):
    cfg = FSN_TINY
    ys = []
    for v in ("1", "0"):
        monkeypatch.setenv("SE_F16_PAIR", v)
        e = make_fsn_engine(cfg)
        ys.append(e.realtime_process(_cuda(audio[:2, :, :6400])).cpu().numpy())
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])
