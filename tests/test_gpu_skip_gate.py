"""GPU tests of the skip gate's arithmetic in the streaming kernels (csrc/skip_p.hip.h: skip_gate_octet, shared by k_skip_p and k_skip_pd;
DESIGN.md 3).  The streaming form takes its per-channel constants as 16-byte rows from LDS, has the activation as a template parameter
and (except with two bf16 planes) computes the norms as subtract-then-FMA and the sigmoid on the hardware exp2 / rcp; the two-launch
form (k_conv_p: statistics, then the kPOutBlend epilogue) keeps the written-out expression with expf and an IEEE division.  Both are
fp32-accurate routes to the same
function, so they must agree within the project's bar between two such routes, 2e-6 relative RMS: outputs, decoder taps and carried
state.  SE_SKIP_MIN_BATCH picks the form (1: streaming at every batch, 100000: two launches); engines as in test_gpu_skip_depth.py."""
import numpy as np
import pytest

from conftest import FULL512, rel_rms, spec_of_variant
from engine_cases import SHORT, SMALL, cuda as _cuda, make_engine, two_call_snapshots, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TAPS = ["dec0", "dec1", "dec2"]
BAR = 2e-6
STREAM, BLEND = "1", "100000"
# (precision, SE_F16_PAIR): the fp16 pair route, the same precision on three bf16 planes, and the two-plane mode
MODES = {"pair": (0, None), "f32_planes": (0, "0"), "p2": (2, None)}


def _state_dict(cfg, variant, scale_residualnorm=None):
    sd = dict(synth.make_state_dict(spec_of_variant(cfg, variant), seed=4))
    if scale_residualnorm is not None:
        k = f"deconvlist.{scale_residualnorm}.residualnorm.weight"
        sd[k] = np.ascontiguousarray(sd[k] * 64.0, dtype=np.float32)
    return sd


def _engine(cfg, min_batch, monkeypatch, mode="pair", variant=0, sd=None):
    precision, f16_pair = MODES[mode]
    env = {"SE_GEMM_SKINNY_ROWS": "0", "SE_SKIP_MIN_BATCH": min_batch}
    return make_engine(cfg, monkeypatch, env if f16_pair is None else dict(env, SE_F16_PAIR=f16_pair), variant=variant, precision=precision,
                       sd=sd if sd is not None else _state_dict(cfg, variant))


@pytest.fixture(scope="module")
def audio():
    return utterances(17, 6400 + 3200, seed=67)


def _run(e, cfg, x):
    """Three segments with flag=False, then two more with flag=True: after each call the output, the decoder taps and the carried state."""
    seg = cfg["segment_length"]
    return [kv for snap in two_call_snapshots(e, cfg, x, (2 * seg, seg + seg // 2), TAPS) for kv in snap.items()]


def _compare(tag, cfg, x, monkeypatch, **kw):
    ref = _run(_engine(cfg, BLEND, monkeypatch, **kw), cfg, x)
    got = _run(_engine(cfg, STREAM, monkeypatch, **kw), cfg, x)
    assert all(np.isfinite(r).all() for _, r in ref) and all(np.abs(r).max() > 0 for n, r in ref if n == "out" or n in TAPS)
    worst = 0.0
    for i, ((name, g), (_, r)) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.isfinite(g).all(), (tag, i, name)
        err = rel_rms(g, r)
        worst = max(worst, err)
        print(f"{tag} {i:2d} {name:5s} rel rms {err:.2e}")
        assert err < BAR, (tag, i, name, err)
    return worst


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,cfg,batch", [
    ("small17", SMALL, 17),
    ("short_no_tile_waves", SHORT, 3),
    ("full512", FULL512, 3),  # KP = 1, 2, 4 and one or two M tiles; 2709, 1365 and 693 positions: a partial last tile
])
def test_streaming_gate_matches_the_blend_epilogue(name, cfg, batch, mode, audio, monkeypatch):
    _compare(f"{name}/{mode}", cfg, audio[:batch], monkeypatch, mode=mode)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_elu_instances_match_the_blend_epilogue(mode, audio, monkeypatch):
    """Variant 1 (CRN_ELU): the ELU instances of the gate at the small shape."""
    _compare(f"small17_elu/{mode}", SMALL, audio[:17], monkeypatch, mode=mode, variant=1)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_saturated_gate_stays_finite_and_within_the_bar(level, audio, monkeypatch):
    """residualnorm weights of one level x 64: with weights of 1 +- 0.25 on a unit-variance input the gate's argument passes +-88
    beyond 1.9 deviations, where exp overflows to inf and rcp(inf) must give an exact 0 (and exp underflows to 0 on the other side)."""
    sd = _state_dict(FULL512, 0, scale_residualnorm=level)
    _compare(f"saturated{level}", FULL512, audio[:3], monkeypatch, sd=sd)


def test_streaming_forward_against_oracle(audio, monkeypatch):
    """Three consecutive forward() frames of FULL512 at 3 streams on the streaming gate, state carried, against the oracle with the
    bars of test_gpu_skip_depth.py's test_batched_forward_against_oracle: output 1e-4; gru tap, enc3 tap and h 2e-5."""
    from oracle import crn_oracle as orc
    cfg, batch = FULL512, 3
    e = _engine(cfg, STREAM, monkeypatch)
    o = orc.CrnOracle(**cfg)
    o.load_state_dict(_state_dict(cfg, 0))
    e.reset(batch)
    o.reset(batch)
    F = cfg["num_freqs"]
    for n in range(3):
        seg = np.ascontiguousarray(audio[:batch, :, n * 1600:n * 1600 + 3200])
        x = o.stft(seg.reshape(-1, 3200)).reshape(batch, 3, F, 21, 2)
        yo = o.forward(x)
        ye = e.forward(_cuda(x)).cpu().numpy()
        r_out, r_gru, r_enc = rel_rms(ye, yo), rel_rms(e.read_tap("gru"), o.tap("gru")), rel_rms(e.read_tap("enc3"), o.tap("enc3"))
        print(f"frame {n}: out {r_out:.2e}  gru tap {r_gru:.2e}  enc3 tap {r_enc:.2e}")
        assert r_out < 1e-4 and r_gru < 2e-5 and r_enc < 2e-5, (n, r_out, r_gru, r_enc)
    assert rel_rms(e.export_state("h"), o.state("h")) < 2e-5
