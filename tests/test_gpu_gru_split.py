"""GPU tests of the split-bf16 GRU step (csrc/gemm.hip.h: k_gru_step_split, SE_GRU_SPLIT): a small configuration that still takes the
plane GEMM route (K dimensions multiples of 32: D = 32 x 17 = 544, hidden 64; SE_GEMM_SKINNY_ROWS=0 so that a small batch runs
k_gemm_p), batches of 17 and 40 streams (more than 16, a partial 32-row tile, two unit groups), utterances of several segments and
a flag=True continuation (the t = 0 hand-over from the fp32 state, ring-slot reuse)."""
import numpy as np
import pytest

from conftest import rel_rms, spec_of
from engine_cases import SMALL as CFG, cuda as _cuda, make_engine as _engine, utterances
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

L1, L2 = 11200, 6400


def _pair(monkeypatch, env_a, env_b, cfg=CFG, precision=0, seed=4):
    """Two engines of one model, each created under its own environment (the knobs are read at creation)."""
    out = []
    for env in (env_a, env_b):
        monkeypatch.setenv("SE_GEMM_SKINNY_ROWS", "0")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(_engine(cfg, seed=seed, precision=precision))
    return out


@pytest.fixture(scope="module")
def audio():
    return utterances(40, L1 + L2, seed=61)


@pytest.mark.parametrize("batch", [17, 40])
def test_split_pipelined_equals_serial(batch, audio, monkeypatch):
    """The multi-layer launch of the pipelined stage against the single-layer launch of the serial path: the same bits."""
    e_ser, e_pip = _pair(monkeypatch, {"SE_GRU_SPLIT": "1", "SE_PIPELINE": "0"}, {"SE_GRU_SPLIT": "1", "SE_PIPELINE": "1"})
    x1, x2 = _cuda(audio[:batch, :, :L1]), _cuda(audio[:batch, :, L1:])
    ref = e_ser.realtime_process(x1).cpu().numpy()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    for _ in range(2):  # twice: ring slots reused across calls
        assert np.array_equal(e_pip.realtime_process(x1).cpu().numpy(), ref)
    ref2 = e_ser.realtime_process(x2, flag=True).cpu().numpy()
    assert np.array_equal(e_pip.realtime_process(x2, flag=True).cpu().numpy(), ref2)
    assert np.array_equal(e_pip.export_state("h"), e_ser.export_state("h"))


@pytest.mark.parametrize("batch", [17, 40])
def test_split_against_fp32_mfma_step(batch, audio, monkeypatch):
    """Against the arithmetic of the fp32-MFMA step kernels: the tolerance the project uses between its two step kernels."""
    e_new, e_old = _pair(monkeypatch, {"SE_GRU_SPLIT": "1"}, {"SE_GRU_SPLIT": "0"})
    for lo, hi, flag in ((0, L1, False), (L1, L1 + L2, True)):
        x = _cuda(audio[:batch, :, lo:hi])
        y_new = e_new.realtime_process(x, flag=flag).cpu().numpy()
        y_old = e_old.realtime_process(x, flag=flag).cpu().numpy()
        r_out = rel_rms(y_new, y_old)
        print(f"batch {batch} flag {flag}: output vs SE_GRU_SPLIT=0 {r_out:.3e}, h vs SE_GRU_SPLIT=0 "
              f"{rel_rms(e_new.export_state('h'), e_old.export_state('h')):.3e}")
        assert r_out < 2e-6, (batch, flag)


@pytest.mark.parametrize("batch", [17, 40])
def test_split_carried_state_against_oracle(batch, audio, monkeypatch):
    """The carried state against the CPU oracle, by the procedure and with the bound of test_gpu_parity.test_forward_stages_vs_oracle:
    three consecutive frames through forward(), state carried, then h within 2e-5.  (After a whole 11 200-sample utterance through
    realtime_process h is 4.07e-5 from the oracle's with SE_GRU_SPLIT=1 and with SE_GRU_SPLIT=0 alike at batch 17: that distance is
    the rest of the network's, not the step kernel's.)"""
    from oracle import crn_oracle as orc
    monkeypatch.setenv("SE_GEMM_SKINNY_ROWS", "0")
    monkeypatch.setenv("SE_GRU_SPLIT", "1")
    e = _engine(CFG, seed=4)
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
        assert rel_rms(ye, yo) < 1e-4, n
    r_h = rel_rms(e.export_state("h"), o.state("h"))
    print(f"batch {batch}: h vs oracle after three frames {r_h:.3e}")
    assert r_h < 2e-5


@pytest.mark.parametrize("case", ["precision2", "hidden16", "batch8"])
def test_split_fallback_keeps_the_bits(case, audio, monkeypatch):
    """Where the new kernel is not eligible (bf16x3 operands, hidden not a multiple of 32, <= 16 streams) SE_GRU_SPLIT=1 changes nothing."""
    cfg = dict(CFG, hidden=16) if case == "hidden16" else CFG
    precision = 2 if case == "precision2" else 0
    batch = 8 if case == "batch8" else 17
    e_on, e_off = _pair(monkeypatch, {"SE_GRU_SPLIT": "1"}, {"SE_GRU_SPLIT": "0"}, cfg=cfg, precision=precision)
    x = _cuda(audio[:batch, :, :L1])
    y_on, y_off = e_on.realtime_process(x).cpu().numpy(), e_off.realtime_process(x).cpu().numpy()
    assert np.abs(y_off).max() > 0
    assert np.array_equal(y_on, y_off)


def test_split_ragged_batch_matches_streams_alone(audio, monkeypatch):
    """Per-stream lengths: the active rows shrink below a full 32-row tile as the short streams end; every stream stays within 2e-6 of
    its run alone (alone it is a batch of one, which takes the <= 16-stream kernel)."""
    monkeypatch.setenv("SE_GEMM_SKINNY_ROWS", "0")
    monkeypatch.setenv("SE_GRU_SPLIT", "1")
    e = _engine(CFG, seed=4)
    lens = [L1 - 1600 * (b % 4) - 37 * (b % 3) for b in range(40)]  # 4 to 7 segments: 40, 30, 20, 10 rows active
    y = e.realtime_process(_cuda(audio[:, :, :L1]), lengths=lens).cpu().numpy()
    e1 = _engine(CFG, seed=4)
    for b in (0, 1, 2, 3, 17, 38, 39):
        alone = e1.realtime_process(_cuda(audio[b:b + 1, :, :lens[b]])).cpu().numpy()
        assert rel_rms(y[b, :lens[b]], alone[0]) < 2e-6, b
        assert np.all(y[b, lens[b]:] == 0), b


def test_split_bits_do_not_depend_on_the_row(audio, monkeypatch):
    """The same stream in different rows of the batch (different waves of a workgroup, different workgroups, the partial last tile)
    gives the same bits: the split-K shares are summed in one order for every row."""
    monkeypatch.setenv("SE_GEMM_SKINNY_ROWS", "0")
    monkeypatch.setenv("SE_GRU_SPLIT", "1")
    e = _engine(CFG, seed=4)
    big = np.ascontiguousarray(np.tile(audio[:2, :, :L1], (20, 1, 1)))
    y = e.realtime_process(_cuda(big)).cpu().numpy()
    for b in range(2, 40):
        assert np.array_equal(y[b], y[b % 2]), b
