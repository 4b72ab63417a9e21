"""GPU parity tests: the HIP engine, called through the C ABI, against the CPU oracle and the
reference-generated golden vectors.  Tolerance: north_star asks waveforms within 1e-4 RMS of the
reference CPU path; with hash weights the outputs have RMS ~1-2, so we assert the *relative* RMS error
(err_rms / ref_rms) < 1e-4, which is the stricter reading."""
import numpy as np
import pytest
import torch

from conftest import FULL400, FULL512, TINY, rel_rms, spec_of
from engine_cases import cuda as _cuda, make_engine as _engine, make_fsn_engine as _fsn_engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _oracle(cfg, seed=0):
    from oracle import crn_oracle as orc
    o = orc.CrnOracle(**cfg)
    o.load_state_dict(synth.make_state_dict(spec_of(cfg), seed=seed))
    return o


@pytest.mark.parametrize("name,cfg", [("400", FULL400), ("512", FULL512)])
def test_stft_istft(golden, name, cfg):
    e = _engine(dict(cfg, num_channels=[2, 2, 2, 2], hidden=16))
    wav = golden["g2_wave"].reshape(-1, 3200)
    sp = e.stft(_cuda(wav)).cpu().numpy().reshape(2, 3, cfg["num_freqs"], 21, 2)
    assert np.abs(sp - golden[f"stft{name}_out"]).max() < 3e-5
    spec_in = synth.hash_tensor("g2.spec" + name, (2, cfg["num_freqs"], 21, 2))
    y = e.istft(_cuda(spec_in)).cpu().numpy()
    assert np.abs(y - golden[f"istft{name}_out"]).max() < 5e-7


def test_stft_zero_and_edges():
    e = _engine(dict(FULL400, num_channels=[2, 2, 2, 2], hidden=16))
    z = e.stft(torch.zeros(3, 3200, device="cuda")).cpu().numpy()
    assert np.all(z == 0)
    from oracle import crn_oracle as orc
    o = orc.CrnOracle(**dict(FULL400, num_channels=[2, 2, 2, 2], hidden=16))
    x = np.zeros((2, 3200), np.float32)
    x[0, 0] = 1.0
    x[1, -1] = -1.0
    assert np.abs(e.stft(_cuda(x)).cpu().numpy() - o.stft(x)).max() < 1e-6


@pytest.mark.parametrize("cfgname", ["tiny", "full400"])
def test_forward_stages_vs_oracle(cfgname):
    """Three consecutive frames (state carried): every tap of forward() against the oracle."""
    cfg = TINY if cfgname == "tiny" else FULL400
    B = 3
    e, o = _engine(cfg), _oracle(cfg)
    mix, _ = synth.synth_utterances(B, 3200 * 3, 3, seed=5)
    e.reset(B)
    o.reset(B)
    F = cfg["num_freqs"]
    for n in range(3):
        seg = mix[:, :, n * 1600:n * 1600 + 3200]
        x = o.stft(seg.reshape(-1, 3200)).reshape(B, 3, F, 21, 2)
        yo = o.forward(x)
        ye = e.forward(_cuda(x)).cpu().numpy()
        L = len(cfg["num_channels"])
        for tap in ["feat"] + [f"enc{i}" for i in range(L)] + ["gru"] + [f"dec{i}" for i in range(L - 1)]:
            r = rel_rms(e.read_tap(tap), o.tap(tap))
            assert r < 2e-5, (cfgname, n, tap, r)
        assert rel_rms(ye, yo) < TOL, (cfgname, n)
    # carried state matches too
    assert rel_rms(e.export_state("h"), o.state("h")) < 2e-5
    for i in range(len(cfg["num_channels"])):
        assert rel_rms(e.export_state(f"buf{i}"), o.state(f"buf{i}")) < 2e-5


def test_tiny_end_to_end_golden(golden):
    e = _engine(TINY)
    mix, _ = synth.synth_utterances(2, 8000 + 4800, 3, seed=7)
    m = _cuda(mix)
    y = e.realtime_process(m[..., :8000].contiguous()).cpu().numpy()
    assert rel_rms(y, golden["tiny_out"]) < TOL
    y2 = e.realtime_process(m[..., 8000:].contiguous(), flag=True).cpu().numpy()
    assert rel_rms(y2, golden["tiny_cont_out"]) < TOL


@pytest.mark.parametrize("tag,cfg", [("full400", FULL400), ("full512", FULL512)])
def test_full_end_to_end_golden(golden, tag, cfg):
    e = _engine(cfg)
    cont = 3200 if tag == "full400" else 0
    mix, clean = synth.synth_utterances(2, 8000 + cont, 3, seed=7)
    m = _cuda(mix)
    y = e.realtime_process(m[..., :8000].contiguous()).cpu().numpy()
    ref = golden[f"{tag}_out"]
    assert rel_rms(y, ref) < TOL
    # SI-SDR of build and reference against the clean signal agree within +-0.02 dB (north_star)
    d = synth.si_sdr(clean[:, :8000], y) - synth.si_sdr(clean[:, :8000], ref)
    assert np.abs(d).max() < 0.02
    if cont:
        y2 = e.realtime_process(m[..., 8000:].contiguous(), flag=True).cpu().numpy()
        assert rel_rms(y2, golden[f"{tag}_cont_out"]) < TOL


def test_full_b1_ragged_golden(golden):
    """BASELINE config 1 (batch 1, ragged length -> gap path), checked against the reference's output."""
    e = _engine(FULL400)
    mix, _ = synth.synth_utterances(1, 5000, 3, seed=11)
    y = e.realtime_process(_cuda(mix)).cpu().numpy()
    assert rel_rms(y, golden["full400_b1_L5000_out"]) < TOL


def test_step_matches_realtime():
    """se_step (per-window API) + host overlap-average == se_realtime_process."""
    from oracle import crn_oracle as orc
    e = _engine(TINY)
    mix, _ = synth.synth_utterances(2, 6400, 3, seed=3)
    y_rt = e.realtime_process(_cuda(mix)).cpu().numpy()
    padded = np.concatenate([np.zeros((2, 3, 1600), np.float32), mix], -1)
    seg, gap = orc.segmentation(padded, 3200)
    N = seg.shape[0] // 2
    seg = seg.reshape(2, N, 3, 3200)
    e.reset(2)
    outs = [e.step(_cuda(seg[:, n])).cpu().numpy() for n in range(N)]
    y = orc.over_add(np.stack(outs, 1), gap)[:, 1600:]
    assert np.abs(y - y_rt).max() < 1e-6


def test_error_conventions():
    from speech_enhancement_mi_amd import engine
    e = _engine(TINY)
    with pytest.raises(RuntimeError, match="before se_reset"):
        e.batch = 2
        e.step(torch.zeros(2, 3, 3200, device="cuda"))
    e.reset(2)
    with pytest.raises(RuntimeError, match="flag=True"):
        e.realtime_process(torch.zeros(3, 3, 3200, device="cuda"), flag=True)
    with pytest.raises(RuntimeError, match="unknown parameter key"):
        e.load_state_dict({"nope.weight": np.zeros(3, np.float32)})
    c = engine.make_config([4, 8, 8, 8], 201, 16, 3200, num_layers=2, n_fft=402)
    with pytest.raises(RuntimeError, match="se_create failed"):
        engine.Engine(c)


def test_dropin_class_matches_reference_golden(golden):
    """The nn.Module shim (same ctor kwargs / state_dict keys as reference CRN.py) end to end on the GPU."""
    from speech_enhancement_mi_amd import TemporalCRN
    m = TemporalCRN(**FULL400)
    sd = synth.make_state_dict(spec_of(FULL400), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to("cuda:0").eval()
    mix, _ = synth.synth_utterances(2, 8000 + 3200, 3, seed=7)
    mt = torch.from_numpy(mix).cuda()
    y = m.realtime_process(mt[..., :8000])
    assert y.shape == (2, 8000) and y.is_cuda
    assert rel_rms(y.cpu().numpy(), golden["full400_out"]) < TOL
    y2 = m.realtime_process(mt[..., 8000:], True)
    assert rel_rms(y2.cpu().numpy(), golden["full400_cont_out"]) < TOL
    # per-frame entry: forward() keeps state, reset() clears it
    o = _oracle(FULL400)
    o.reset(2)
    x = o.stft(mix[:, :, :3200].reshape(-1, 3200)).reshape(2, 3, 201, 21, 2)
    m.reset()
    y_f = m(torch.from_numpy(x).cuda())
    assert rel_rms(y_f.cpu().numpy(), o.forward(x)) < TOL
    # a weight update is picked up (version counters)
    with torch.no_grad():
        m.gru.norm.bias.add_(0.5)
    y3 = m.realtime_process(mt[..., :8000])
    assert rel_rms(y3.cpu().numpy(), golden["full400_out"]) > 1e-3


def test_full_size_batch256_properties():
    """BASELINE configs[1] size (B=256 streams, 512-pt): size-independent properties instead of an oracle run.
    (i) batch independence: stream i of the big batch equals the same utterance processed in a batch of 4
        (all norms/state are per stream) - this is also what makes stream sharding exact;
    (ii) prefix consistency: the output for a prefix equals the full output until the last,
        zero-padded segment;  (iii) repeatability after reset;  (iv) finite output."""
    e = _engine(FULL512)
    L = 16000
    base, _ = synth.synth_utterances(4, L, 3, seed=21)
    big = np.ascontiguousarray(np.tile(base, (64, 1, 1)))
    y_big = e.realtime_process(_cuda(big)).cpu().numpy()
    assert np.isfinite(y_big).all()
    y_small = e.realtime_process(_cuda(base)).cpu().numpy()
    for i in (0, 1, 2, 3, 100, 255):
        assert rel_rms(y_big[i], y_small[i % 4]) < 2e-6, i
    y_again = e.realtime_process(_cuda(big)).cpu().numpy()
    assert np.array_equal(y_again, y_big)  # deterministic: no atomics, fixed reduction order
    y_prefix = e.realtime_process(_cuda(base[..., :9600])).cpu().numpy()
    # segments fully inside the prefix (all but the zero-padded tail) agree: first 9600-1600 samples
    assert rel_rms(y_prefix[:, :8000], y_small[:, :8000]) < 2e-6


@pytest.mark.parametrize("batch", [3, 64, 256])
def test_stage_pipeline_equals_serial(batch, monkeypatch):
    """se_realtime_process runs the encoder / recurrent / decoder stages of successive segments on three HIP streams
    (ring of 4 activation slots).  The overlap must not change a single bit: compare with the same
    engine built with SE_PIPELINE=0 (one stream, stages back to back), twice (slot reuse across calls), and once
    more with a carried state (flag=True continues from the ring slot the previous call ended on).
    SE_GRU_DIRECT pins the GRU step kernel: by default the overlapped stage uses the small-footprint kernel and the
    single-stream path the LDS-slice kernel, which differ in summation order (covered by the tolerance test below)."""
    monkeypatch.setenv("SE_GRU_DIRECT", "1")
    monkeypatch.setenv("SE_PIPELINE", "0")
    e_serial = _engine(FULL512, seed=5)
    monkeypatch.setenv("SE_PIPELINE", "1")
    e_piped = _engine(FULL512, seed=5)
    mix, _ = synth.synth_utterances(batch, 11200, 3, seed=31)
    x = _cuda(mix)
    ref = e_serial.realtime_process(x).cpu().numpy()
    for _ in range(2):
        assert np.array_equal(e_piped.realtime_process(x).cpu().numpy(), ref)
    x2 = _cuda(mix[..., :6400])
    ref2 = e_serial.realtime_process(x2, flag=True).cpu().numpy()
    assert np.array_equal(e_piped.realtime_process(x2, flag=True).cpu().numpy(), ref2)


def test_stage_pipeline_long_utterance_crosses_chunks(monkeypatch):
    """More than kPipeChunk = 64 segments (7 s -> 72 segments): the pipelined path drains and re-forks at the chunk
    boundary and reuses its spectrum / mask staging buffers; ragged sub-batches of the (i)STFT launches included."""
    monkeypatch.setenv("SE_GRU_DIRECT", "1")
    monkeypatch.setenv("SE_PIPELINE", "0")
    e_serial = _engine(FULL400, seed=7)
    monkeypatch.setenv("SE_PIPELINE", "1")
    e_piped = _engine(FULL400, seed=7)
    mix, _ = synth.synth_utterances(2, 16000 * 7 + 123, 3, seed=35)
    x = _cuda(mix)
    ref = e_serial.realtime_process(x).cpu().numpy()
    assert np.array_equal(e_piped.realtime_process(x).cpu().numpy(), ref)


def test_stage_pipeline_default_kernels_within_tolerance(monkeypatch):
    """Default configuration: pipelined (k_gru_step in the overlapped stage) vs single stream (k_gru_step2)."""
    monkeypatch.setenv("SE_PIPELINE", "0")
    e_serial = _engine(FULL512, seed=5)
    monkeypatch.setenv("SE_PIPELINE", "1")
    e_piped = _engine(FULL512, seed=5)
    mix, _ = synth.synth_utterances(8, 11200, 3, seed=33)
    x = _cuda(mix)
    assert rel_rms(e_piped.realtime_process(x).cpu().numpy(), e_serial.realtime_process(x).cpu().numpy()) < 2e-6


def test_stage_pipeline_equals_serial_variants(monkeypatch):
    """Same bit-exactness for the CRN_ELU (pre-conv chain, gated pairs) and student (hidden 128) pipelines."""
    monkeypatch.setenv("SE_GRU_DIRECT", "0")
    for cfg, variant in ((FULL400, 1), (STUDENT400, 2)):
        monkeypatch.setenv("SE_PIPELINE", "0")
        e_serial = _engine(cfg, variant=variant, seed=6)
        monkeypatch.setenv("SE_PIPELINE", "1")
        e_piped = _engine(cfg, variant=variant, seed=6)
        mix, _ = synth.synth_utterances(16, 9600, 3, seed=32)
        x = _cuda(mix)
        ref = e_serial.realtime_process(x).cpu().numpy()
        assert np.array_equal(e_piped.realtime_process(x).cpu().numpy(), ref), variant


def test_reset_single_stream_keeps_the_others():
    """se_reset_stream (streams joining / leaving the batch): after resetting stream 1 only, stream 1 behaves
    like a freshly reset engine and stream 0 like an engine that was never touched."""
    cfg = FULL400
    e, e_fresh, e_cont = _engine(cfg, seed=3), _engine(cfg, seed=3), _engine(cfg, seed=3)
    a, _ = synth.synth_utterances(2, 3200 * 3, 3, seed=41)
    bnew, _ = synth.synth_utterances(1, 3200 * 2, 3, seed=42)
    e.reset(2); e_cont.reset(2); e_fresh.reset(1)
    for k in range(3):  # both streams hear utterance a
        w = _cuda(a[:, :, 3200 * k:3200 * (k + 1)])
        e.step(w); e_cont.step(w)
    e.reset_stream(1)
    for k in range(2):  # stream 0 goes on with (a repeat of) a, stream 1 is a new caller with bnew
        w0 = a[:1, :, 3200 * k:3200 * (k + 1)]
        w1 = bnew[:, :, 3200 * k:3200 * (k + 1)]
        y = e.step(_cuda(np.concatenate([w0, w1], 0))).cpu().numpy()
        y_cont = e_cont.step(_cuda(np.concatenate([w0, w0], 0))).cpu().numpy()
        y_fresh = e_fresh.step(_cuda(w1)).cpu().numpy()
        assert rel_rms(y[1], y_fresh[0]) < 2e-6, k
        assert np.array_equal(y[0], y_cont[0]), k
    with pytest.raises(RuntimeError):
        e.reset_stream(2)


def test_fft_kernels_exact_under_coexecution(monkeypatch):
    """Regression test for the packed-FP32 co-residency fault (csrc/se_aux.hip): the STFT / iSTFT of one
    engine must stay bit-exact while an unrelated engine runs its MFMA kernels on another stream.  Before the FFT
    kernels were built without packed-FP32 instructions 30-40 % of these launches returned wrong frames."""
    monkeypatch.setenv("SE_PIPELINE", "0")
    e_a, e_b = _engine(FULL512, seed=1), _engine(FULL512, seed=2)
    mix, _ = synth.synth_utterances(64, 16000, 3, seed=3)
    x = _cuda(mix)
    seg = torch.randn(96, 3200, device="cuda")
    ref = e_b.stft(seg).clone()
    ref_i = e_b.istft(ref).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for it in range(3):  # iteration 0 allocates (which serialises the streams); 1 and 2 overlap for real
        outs, outs_i = [], []
        with torch.cuda.stream(s1):
            e_a.realtime_process(x)
        with torch.cuda.stream(s2):
            for _ in range(60):
                outs.append(e_b.stft(seg))
                outs_i.append(e_b.istft(ref))
        torch.cuda.synchronize()
        assert all(torch.equal(o, ref) for o in outs), it
        assert all(torch.equal(o, ref_i) for o in outs_i), it


def test_istft_stft_roundtrip_full_batch():
    """Size-independent property at full batch: iSTFT(STFT(x)) == x on the samples covered by complete frames."""
    e = _engine(dict(FULL512, num_channels=[2, 2, 2, 2], hidden=16))
    x = torch.rand(768, 3200, device="cuda") - 0.5
    y = e.istft(e.stft(x))
    assert float((y - x).abs().max()) < 2e-6


# ---- a12 / a13: CRN_ELU.py and the distilled-student architecture ------------------------------------------------
from conftest import STUDENT400, spec_of_variant  # noqa: E402


def _oracle_v(cfg, variant, seed=0):
    from oracle import crn_oracle as orc
    o = orc.CrnOracle(**cfg, variant=variant)
    o.load_state_dict(synth.make_state_dict(spec_of_variant(cfg, variant), seed=seed))
    return o


@pytest.mark.parametrize("name,cfg,variant", [("elu_tiny", TINY, 1), ("student_tiny", TINY, 2), ("elu_full", FULL400, 1),
                                              ("student_full", STUDENT400, 2)])
def test_variant_forward_stages_vs_oracle(name, cfg, variant):
    B = 2
    e, o = _engine(cfg, variant=variant), _oracle_v(cfg, variant)
    mix, _ = synth.synth_utterances(B, 3200 * 3, 3, seed=5)
    e.reset(B)
    o.reset(B)
    F, L = cfg["num_freqs"], len(cfg["num_channels"])
    for n in range(3):
        seg = mix[:, :, n * 1600:n * 1600 + 3200]
        x = o.stft(seg.reshape(-1, 3200)).reshape(B, 3, F, 21, 2)
        yo = o.forward(x)
        ye = e.forward(_cuda(x)).cpu().numpy()
        for tap in ["feat"] + [f"enc{i}" for i in range(L)] + ["gru"] + [f"dec{i}" for i in range(L - 1)]:
            r = rel_rms(e.read_tap(tap), o.tap(tap))
            assert r < 2e-5, (name, n, tap, r)
        assert rel_rms(ye, yo) < TOL, (name, n)
    assert rel_rms(e.export_state("h"), o.state("h")) < 2e-5
    for i in range(L):
        assert rel_rms(e.export_state(f"buf{i}"), o.state(f"buf{i}")) < 2e-5
    for i in range(3):
        assert rel_rms(e.export_state(f"pbuf{i}"), o.state(f"pbuf{i}")) < 2e-5


@pytest.mark.parametrize("tag,cfg,variant,L,cont", [("elu_tiny", TINY, 1, 8000, 4800), ("student_tiny", TINY, 2, 8000, 4800),
                                                    ("elu_full400", FULL400, 1, 6400, 0), ("student_full400", STUDENT400, 2, 6400, 0)])
def test_variant_end_to_end_golden(vgolden, tag, cfg, variant, L, cont):
    """Against the outputs of the genuine reference CRN_ELU.py / distillation_crn.py modules."""
    e = _engine(cfg, variant=variant)
    mix, _ = synth.synth_utterances(2, L + cont, 3, seed=7)
    m = _cuda(mix)
    y = e.realtime_process(m[..., :L].contiguous()).cpu().numpy()
    assert rel_rms(y, vgolden[f"{tag}_out"]) < TOL
    if cont:
        y2 = e.realtime_process(m[..., L:].contiguous(), flag=True).cpu().numpy()
        assert rel_rms(y2, vgolden[f"{tag}_cont_out"]) < TOL


def test_variant_dropin_classes(vgolden):
    from speech_enhancement_mi_amd import crn_elu, distillation_crn
    mix, _ = synth.synth_utterances(2, 6400, 3, seed=7)
    mt = torch.from_numpy(mix).cuda()
    m1 = crn_elu.TemporalCRN(**FULL400)
    m1.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of_variant(FULL400, 1)).items()}, strict=True)
    y1 = m1.cuda().realtime_process(mt)
    assert rel_rms(y1.cpu().numpy(), vgolden["elu_full400_out"]) < TOL
    m2 = distillation_crn.TemporalCRN(**STUDENT400)
    assert abs(sum(p.numel() for p in m2.parameters()) / 1e6 - 0.812) < 0.005  # README.md:58 "0.81 MB"
    m2.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of_variant(STUDENT400, 2)).items()}, strict=True)
    m2.return_features = False  # inference: skip the distillation feature taps (covered by tests/test_gpu_round2.py)
    y2, feats = m2.cuda().realtime_process(mt, flag=False)  # predict_distillation.py:84 unpacks a pair
    assert feats is None
    assert rel_rms(y2.cpu().numpy(), vgolden["student_full400_out"]) < TOL


# ---- which CRN geometries se_reset accepts (crn_geometry_supported in se_engine.hip) ----------------------------------------
@pytest.mark.parametrize("cfg,variant,accepted", [
    (TINY, 0, True), (FULL400, 0, True), (FULL512, 0, True), (STUDENT400, 2, True),
    (dict(FULL400, num_channels=[2, 2, 2, 2], hidden=16), 0, True),
    (dict(FULL400, num_channels=[128, 128, 128, 128]), 0, False),  # a skip connection's 1x1 pair: 2 x 128 GEMM rows
    (dict(FULL400, num_channels=[16, 32, 64, 40]), 1, False),      # CRN_ELU gated pair of 40 channels: 80 rows = 3 row tiles
    (dict(FULL400, num_channels=[16, 32, 64, 40]), 0, True),       # the same channels without the gated pair
    (dict(FULL400, num_inputs=5), 1, False),                       # pre-conv blocks: at most 8 feature channels
], ids=["tiny", "full400", "full512", "student400", "ch2_tiny", "crn_128x4", "elu_c40", "crn_c40", "elu_5_inputs"])
def test_crn_geometry_acceptance(cfg, variant, accepted):
    e = _engine(cfg, variant=variant)
    if accepted:
        e.reset(2)
    else:
        with pytest.raises(RuntimeError, match=r"se_engine error -1:"):  # SE_ERR_ARG
            e.reset(2)


# ---- a14 / a15: FullSubNet ----------------------------------------------------------------------------------------------
from conftest import FSN_FULL, FSN_TINY, fsn_spec  # noqa: E402


def _fsn_oracle(cfg):
    from oracle import crn_oracle as orc
    o = orc.FsnOracle(**cfg)
    o.load_state_dict(synth.make_state_dict(fsn_spec(cfg), seed=0))
    return o


@pytest.mark.parametrize("name,cfg,B", [("tiny", FSN_TINY, 3), ("full", FSN_FULL, 1)])
def test_fsn_forward_vs_oracle(name, cfg, B):
    """Three consecutive segments (LSTM state and both running-mean norms carried): compressed mask, full-band output
    and running means against the oracle."""
    from oracle import crn_oracle as orc
    e, o = _fsn_engine(cfg), _fsn_oracle(cfg)
    sig = orc.CrnOracle(**dict(FULL400, num_channels=[2, 2, 2, 2], hidden=4))
    mix, _ = synth.synth_utterances(B, 3200 * 3, 3, seed=5)
    e.reset(B)
    o.reset(B)
    for n in range(3):
        seg = mix[:, :, n * 1600:n * 1600 + 3200]
        sp = sig.stft(seg.reshape(-1, 3200)).reshape(B, 3, 201, 21, 2)
        x = np.concatenate([sp[..., 0], sp[..., 1]], axis=1)  # [B, 2M, F, T], fullsubnet.py:835-844
        co = o.forward(x)
        ce = e.forward(_cuda(x)).cpu().numpy()
        fb_e = e.read_tap("fb_out").reshape(B, 21, 201).transpose(0, 2, 1)
        assert rel_rms(fb_e, o.tap("fb_out").reshape(B, 201, 21)) < 2e-5, (name, n)
        assert rel_rms(e.read_tap("mean_fb"), o.tap("mean_fb")) < 1e-6 and rel_rms(e.read_tap("mean_sb"), o.tap("mean_sb")) < 1e-5
        assert rel_rms(ce, co) < 5e-5, (name, n, rel_rms(ce, co))


def test_fsn_tiny_end_to_end_golden(fgolden):
    e = _fsn_engine(FSN_TINY)
    mix, _ = synth.synth_utterances(2, 8000 + 4800, 3, seed=7)
    m = _cuda(mix)
    y = e.realtime_process(m[..., :8000].contiguous()).cpu().numpy()
    assert rel_rms(y, fgolden["fsn_tiny_out"]) < TOL
    y2 = e.realtime_process(m[..., 8000:].contiguous(), flag=True).cpu().numpy()
    assert rel_rms(y2, fgolden["fsn_tiny_cont_out"]) < TOL


def test_fsn_full_end_to_end_golden_and_dropin(fgolden):
    """Reference-size FullSubNet (config.yaml:153-172) against the output of the genuine reference class."""
    from speech_enhancement_mi_amd.fullsubnet import FullSubNet
    m = FullSubNet(**FSN_FULL)
    sd = synth.make_state_dict(fsn_spec(FSN_FULL), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    mix, clean = synth.synth_utterances(1, 4800, 3, seed=7)
    src = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    y, crm, s, x = m.cuda().realtime_process(torch.from_numpy(mix).cuda(), src, flag=False, train=False)  # predict_fullsubnet.py:75
    assert crm is None and s is None and x is None
    assert rel_rms(y.cpu().numpy(), fgolden["fsn_full_out"]) < TOL


# ---- edge cases the reference's padding logic defines (utility.py:312-336): very short, ragged and boundary lengths ----------
@pytest.mark.parametrize("L", [1, 7, 1599, 1600, 1601, 3199, 3200, 3201, 4800, 6400])
def test_edge_lengths_vs_oracle(L):
    e, o = _engine(TINY), _oracle(TINY)
    mix, _ = synth.synth_utterances(2, max(L, 64), 3, seed=13)
    mix = np.ascontiguousarray(mix[..., :L])
    y = e.realtime_process(_cuda(mix)).cpu().numpy()
    ref = o.realtime_process(mix)
    assert y.shape == (2, L)
    assert np.abs(y - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), L


def test_large_batch_and_long_utterance_smoke():
    """Maximum sizes the benchmark uses and beyond: B = 512 streams, 3.75 s (the reference's max_length, config.yaml:11)."""
    e = _engine(FULL400)
    base, _ = synth.synth_utterances(2, 60000, 3, seed=17)
    big = np.ascontiguousarray(np.tile(base, (256, 1, 1)))
    y = e.realtime_process(_cuda(big)).cpu().numpy()
    assert y.shape == (512, 60000) and np.isfinite(y).all()
    assert np.array_equal(y[0], y[2]) and np.array_equal(y[1], y[511])


# ---- fp16 operand mode (BASELINE config 5: the student in fp16) ---------------------------------------------------------
@pytest.mark.parametrize("cfg,variant", [(STUDENT400, 2), (FULL512, 0)])
def test_fp16_operand_mode_close_to_fp32(cfg, variant):
    """precision = 1: convolutions and dense layers take fp16 MFMA operands (11 mantissa bits) with fp32 accumulation,
    storage / norms / recurrence stay fp32.  Not the 1e-4 bar of the fp32 path: the test pins what fp16 operands cost
    against the fp32-accurate engine on the same weights and input - relative RMS < 3e-3 and SI-SDR within 0.1 dB of the
    fp32 engine's SI-SDR against the clean reference signal (hash weights give SI-SDRs of -5 ... -31 dB, where the measure
    is very sensitive; measured differences are 0.001 ... 0.05 dB)."""
    e32, e16 = _engine(cfg, variant=variant, precision=0, seed=4), _engine(cfg, variant=variant, precision=1, seed=4)
    mix, clean = synth.synth_utterances(8, 16000, 3, seed=51)
    x = _cuda(mix)
    y32, y16 = e32.realtime_process(x).cpu().numpy(), e16.realtime_process(x).cpu().numpy()
    assert np.isfinite(y16).all()
    err = rel_rms(y16, y32)
    assert err < 3e-3, err
    s32 = np.array([synth.si_sdr(y32[i], clean[i]) for i in range(8)])
    s16 = np.array([synth.si_sdr(y16[i], clean[i]) for i in range(8)])
    assert np.abs(s32 - s16).max() < 0.1, (s32, s16)


def test_half_model_selects_fp16_engine():
    """The PyTorch idiom: model.half() -> the drop-in class builds its engine with precision = 1."""
    from speech_enhancement_mi_amd.distillation_crn import TemporalCRN as Student
    m = Student(**STUDENT400)
    sd = synth.make_state_dict(spec_of_variant(STUDENT400, 2), seed=9)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.cuda()
    m.return_features = False
    mix, _ = synth.synth_utterances(2, 8000, 3, seed=52)
    y32 = m.realtime_process(_cuda(mix))
    y32 = (y32[0] if isinstance(y32, tuple) else y32).float().cpu().numpy()
    m = m.half()
    y16 = m.realtime_process(_cuda(mix).half())
    y16 = (y16[0] if isinstance(y16, tuple) else y16).float().cpu().numpy()
    assert m._eng_precision == 1
    # .half() also rounds the stored weights (incl. the GRU's and the norms') and the input to fp16: a little more than the
    # 3e-3 of fp16 operands alone
    assert 1e-7 < rel_rms(y16, y32) < 1e-2
