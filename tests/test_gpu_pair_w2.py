"""GPU tests of the fp16 pair's two stored weight planes (csrc/split_f16pair.h).  By default a pair weight is
stored as (w_lo, w_hi) and k_gemm_p, k_conv_p, k_skip_p and the split GRU step make 2^11 w_hi from the w_hi fragment with a packed fp16
multiply; SE_PAIR_W3=1 keeps the three stored planes (2^11 w_hi, w_lo, w_hi) and the instances that read them.  The same operand bits
go into the same MFMAs in the same order, so the two routes must agree BIT FOR BIT: outputs, every tap and the carried state.
Shapes and helpers of test_gpu_f16_pair_conv.py: channels [8, 8, 16, 32], hidden 64, 512-point, SE_GEMM_SKINNY_ROWS=0; 17 streams
with SE_SKIP_MIN_BATCH=1 (k_skip_p) and 40 without (the two-launch kPOutBlend form); FULL512 at 4 streams; 6400 samples with flag=False,
then 4800 with the carried state."""
import numpy as np
import pytest
import torch

from conftest import FULL512, STUDENT400, TINY, spec_of
from engine_cases import SMALL as CFG, cuda as _cuda, make_engine, snapshot, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

L1, L2 = 6400, 4800
TAPS = ["feat", "enc0", "enc1", "enc2", "enc3", "gru", "dec0", "dec1", "dec2"]
SKIP_STREAM = {"SE_SKIP_MIN_BATCH": "1"}
W3 = {"SE_PAIR_W3": "1"}
# profile-record names of the instances that read two stored planes / three (the convolutions keep one name for both)
NAMES_W2 = {"k_gemm_p_w2", "k_skip_p_w2", "k_gru_step_split_w2", "k_gru_step_split_multi_w2"}
NAMES_W3 = {"k_gemm_p", "k_skip_p", "k_gru_step_split", "k_gru_step_split_multi"}


def _engine(cfg, env, monkeypatch, seed=4, precision=0, variant=0, sd=None):
    """An engine created under `env` (the knobs are read at creation; every engine here is on the plane GEMM route)."""
    return make_engine(cfg, monkeypatch, dict({"SE_GEMM_SKINNY_ROWS": "0"}, **env), seed=seed, precision=precision, variant=variant, sd=sd)


@pytest.fixture(scope="module")
def audio():
    return utterances(40, L1 + L2, seed=61)


def _snapshot(e, cfg, y):
    return snapshot(e, cfg, y, TAPS)


def _kernels(e, x):
    """Profile-record kernel names of one more call (flag=True: the state moves on in both engines alike)."""
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # timed events: on a stream of their own (bench.py)
        e.profile(True)
        e.realtime_process(x, flag=True)
        recs = e.profile_read()
        e.profile(False)
    torch.cuda.synchronize()
    return {r["kernel"] for r in recs}


def _same_bits(cfg, batch, env, audio, monkeypatch, sd=None):
    e_w2, e_w3 = _engine(cfg, env, monkeypatch, sd=sd), _engine(cfg, dict(env, **W3), monkeypatch, sd=sd)
    for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
        x = _cuda(audio[:batch, :, lo:hi])
        w2 = _snapshot(e_w2, cfg, e_w2.realtime_process(x, flag=flag).cpu().numpy())
        w3 = _snapshot(e_w3, cfg, e_w3.realtime_process(x, flag=flag).cpu().numpy())
        assert np.isfinite(w3["out"]).all() and np.abs(w3["out"]).max() > 0
        for k in w2:
            d = np.abs(w2[k].astype(np.float64) - w3[k])
            print(f"{env} batch {batch} flag {flag} {k}: max abs diff {d.max():.3g}")
            assert np.array_equal(w2[k], w3[k]), (env, batch, flag, k, float(d.max()))
    # the routes really differ: the default runs the two-plane instances (two thirds of the weight bytes) and none of the
    # three-plane ones, SE_PAIR_W3=1 the reverse - and both are on the pair format at all (a failed range guard would run neither)
    x = _cuda(audio[:batch, :, :L2])
    k_w2, k_w3 = _kernels(e_w2, x), _kernels(e_w3, x)
    print(f"default: {sorted(k_w2 & (NAMES_W2 | NAMES_W3))}  SE_PAIR_W3=1: {sorted(k_w3 & (NAMES_W2 | NAMES_W3))}")
    assert "k_gemm_p_w2" in k_w2 and not (k_w2 & NAMES_W3), k_w2
    assert "k_gemm_p" in k_w3 and not (k_w3 & NAMES_W2), k_w3
    return k_w2


SHAPES = {"small17_stream": (CFG, 17, SKIP_STREAM), "small40": (CFG, 40, {}), "full512": (FULL512, 4, SKIP_STREAM)}
VARIANTS = [{}, {"SE_DEC_PAIR": "0"}, {"SE_PIPELINE": "0"}, {"SE_PIPELINE": "0", "SE_GRU_SPLIT": "1"}]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()) or "default")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_stored_planes_give_the_bits_of_three(shape, variant, audio, monkeypatch):
    """SE_DEC_PAIR 1 (default) and 0, SE_PIPELINE 1 (default) and 0 - with SE_GRU_SPLIT=1 the single-layer split GRU step as well (above 16
    streams) - at each shape: bit-equal outputs, taps feat, enc0-3, gru, dec0-2 and exported state h, buf*."""
    cfg, batch, env = SHAPES[shape]
    names = _same_bits(cfg, batch, dict(env, **variant), audio, monkeypatch)
    if env is SKIP_STREAM:
        assert "k_skip_p_w2" in names, names
    if variant.get("SE_GRU_SPLIT") == "1" and batch > 16:  # (the pipelined default runs the multi-layer form of the same body)
        assert names & {"k_gru_step_split_w2", "k_gru_step_split_multi_w2"}, names


def _edited_state_dict():
    """W_hh, one convolution weight, one residual.weight and the fc weight: a tenth of the elements at 1e-7 .. 1e-4 (an fp16-subnormal high
    part), a tenth at exact +-0, a few at +-15.9 (2^11 w_hi just below the top of fp16) - where a wrong device scale would show."""
    rng = np.random.default_rng(7)
    sd = {k: np.array(v, dtype=np.float32, copy=True) for k, v in synth.make_state_dict(spec_of(CFG), seed=4).items()}
    done = []
    for keys, big in ((("gru.sequence_model.weight_hh_l0",), 6), (("convlist.2.conv.weight", "convlist.2.net.0.weight"), 6),
                      (("deconvlist.1.residual.weight",), 2), (("gru.fc_output_layer.weight",), 6)):
        edit = None
        for k in keys:  # (one tensor under the reference's two names gets the same edit)
            if k not in sd:
                continue
            w = sd[k].reshape(-1)
            if edit is None:
                idx = rng.permutation(w.size)
                n = w.size // 10
                tiny = np.exp(rng.uniform(np.log(1e-7), np.log(1e-4), n)).astype(np.float32) * rng.choice([-1.0, 1.0], n).astype(np.float32)
                zero = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
                top = np.float32(15.9) * rng.choice([-1.0, 1.0], big).astype(np.float32)
                edit = (idx, n, tiny, zero, top)
            idx, n, tiny, zero, top = edit
            w[idx[:n]] = tiny
            w[idx[n:2 * n]] = zero
            w[idx[2 * n:2 * n + big]] = top
            done.append(k)
    assert len({"gru.sequence_model.weight_hh_l0", "deconvlist.1.residual.weight", "gru.fc_output_layer.weight"} & set(done)) == 3 and len(done) >= 4, done
    return sd


@pytest.mark.parametrize("shape", ["small17_stream", "small40"])
def test_subnormal_zero_and_large_weights(shape, audio, monkeypatch):
    cfg, batch, env = SHAPES[shape]
    _same_bits(cfg, batch, env, audio, monkeypatch, sd=_edited_state_dict())


@pytest.mark.parametrize("case", ["precision1", "precision2", "crn_elu", "student", "guard_fails"])
def test_knob_leaves_other_routes_alone(case, audio, monkeypatch):
    """fp16 operands, bf16x3, CRN_ELU, the student and a checkpoint that fails the range guard do not run the pair format: SE_PAIR_W3
    either way, the same bits (the eligibility cases of test_gpu_f16_pair.py)."""
    cfg, precision, variant = {"precision1": (CFG, 1, 0), "precision2": (CFG, 2, 0), "crn_elu": (TINY, 0, 1), "student": (STUDENT400, 0, 2),
                               "guard_fails": (CFG, 0, 0)}[case]
    sd = None
    if case == "guard_fails":
        sd = {k: np.array(v, dtype=np.float32, copy=True) for k, v in synth.make_state_dict(spec_of(cfg), seed=0).items()}
        for k in ("convlist.2.conv.weight", "convlist.2.net.0.weight"):
            if k in sd:
                sd[k].reshape(-1)[5] = 40.0
    x = _cuda(audio[:17 if cfg is CFG else 3, :, :L1])
    ys = [_engine(cfg, env, monkeypatch, seed=0, precision=precision, variant=variant, sd=sd).realtime_process(x).cpu().numpy()
          for env in ({"SE_PAIR_W3": "0"}, {"SE_PAIR_W3": "1"})]
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1])
