"""GPU tests of the batched streaming skip gate (csrc/skip_p.hip.h: k_skip_pd, SE_SKIP_DEPTH).  The batched kernel issues
its loads earlier and reads `res` once where a wave's tiles fit one batch; every MFMA, every sum and their order are those of k_skip_p,
so each value of the knob must give the BITS of SE_SKIP_DEPTH=0 (the one-tile-ahead loop): outputs, decoder taps and carried state.
Engines as in test_gpu_f16_pair.py: SE_GEMM_SKINNY_ROWS=0, SE_SKIP_MIN_BATCH=1 (k_skip_p / k_skip_pd at every batch), knobs set
before creation; three segments with flag=False, then two more with flag=True."""
import numpy as np
import pytest

from conftest import FULL512, rel_rms, spec_of
from engine_cases import SHORT, SMALL, cuda as _cuda, make_engine, two_call_snapshots, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TAPS = ["dec0", "dec1", "dec2"]
# the one-ahead loop (the reference); several batches (one and two tiles); the capacity on every level; the default (the capacity on the
# levels with KP = 1 and 4, the one-ahead loop on those with KP = 2)
DEPTHS = ["0", "1", "2", "64", None]


def _engine(cfg, depth, monkeypatch, precision=0):
    env = {"SE_GEMM_SKINNY_ROWS": "0", "SE_SKIP_MIN_BATCH": "1"}
    return make_engine(cfg, monkeypatch, env if depth is None else dict(env, SE_SKIP_DEPTH=depth), precision=precision, seed=4)


@pytest.fixture(scope="module")
def audio():
    return utterances(17, 6400 + 3200, seed=67)


def _run(e, cfg, x):
    """Three segments with flag=False, then two more with flag=True: after each call the output, the decoder taps and the carried state."""
    seg = cfg["segment_length"]
    return [a for snap in two_call_snapshots(e, cfg, x, (2 * seg, seg + seg // 2), TAPS) for a in snap.values()]


@pytest.mark.parametrize("name,cfg,batch,precision", [
    ("full512", FULL512, 3, 0),       # fp16 pair planes: KP = 1, 2, 4 and one or two M tiles; 2709, 1365 and 693 positions: a partial last tile
    ("full512_bf16x3", FULL512, 3, 2),
    ("full512_f16", FULL512, 3, 1),
    ("small17", SMALL, 17, 0),
    ("short_no_tile_waves", SHORT, 3, 0),
])
def test_every_depth_gives_the_bits_of_the_one_ahead_loop(name, cfg, batch, precision, audio, monkeypatch):
    x = audio[:batch]
    ref = _run(_engine(cfg, DEPTHS[0], monkeypatch, precision), cfg, x)
    assert all(np.isfinite(r).all() for r in ref) and np.abs(ref[0]).max() > 0 and all(np.abs(r).max() > 0 for r in ref[1:4])
    for depth in DEPTHS[1:]:
        got = _run(_engine(cfg, depth, monkeypatch, precision), cfg, x)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g.shape == r.shape and np.array_equal(g, r), (name, depth, i, float(np.abs(g - r).max()))


def test_batched_forward_against_oracle(audio, monkeypatch):
    """Three consecutive forward() frames of FULL512 at 3 streams with the state carried, the default depth (test_gpu_f16_pair.py's
    test_pair_route_forward_against_oracle runs the small configuration): output within 1e-4, the decoder-input tap, the deepest
    encoder tap and h within 2e-5 of the oracle."""
    from oracle import crn_oracle as orc
    cfg, batch = FULL512, 3
    e = _engine(cfg, None, monkeypatch)
    o = orc.CrnOracle(**cfg)
    o.load_state_dict(synth.make_state_dict(spec_of(cfg), seed=4))
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
