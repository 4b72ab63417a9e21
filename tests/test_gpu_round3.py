"""GPU tests added in round 3: the persistent training GRU (one launch per layer and direction), the weight-reload route
fix, wide training batches, config 5 in its named dtype at size, and the
hand-written norm / pointwise / signal kernels of the training step."""
import numpy as np
import pytest
import torch

from conftest import FULL400, FULL512, STUDENT400, TINY, rel_rms, spec_of, spec_of_variant
from engine_cases import cuda as _cuda, make_engine as _engine
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---- a weight reload must not switch the plane GEMM route back on for a small batch ---------------------
def test_weight_reload_keeps_small_batch_gemm_route():
    """reset(B=1) puts the bottleneck GEMMs on the skinny route (no plane buffers allocated); se_load_param clears
    weights_ready and the next step re-plans.  The re-plan used to set gemm_p from the capability alone -> k_gemm_p on null
    plane buffers.  Now: step, reload the same weights, step again == a fresh engine fed the same two windows."""
    sd = synth.make_state_dict(spec_of(FULL512), seed=5)
    mix, _ = synth.synth_utterances(1, 6400, 3, seed=13)
    w0, w1 = _cuda(mix[:, :, :3200]), _cuda(mix[:, :, 3200:])
    a, b = _engine(FULL512, seed=5), _engine(FULL512, seed=5)
    a.reset(1); b.reset(1)
    ya0 = a.step(w0).cpu().numpy()
    a.load_state_dict(sd)          # optimizer step / load_state_dict on the drop-in class does exactly this
    ya1 = a.step(w1).cpu().numpy()
    yb0 = b.step(w0).cpu().numpy()
    yb1 = b.step(w1).cpu().numpy()
    assert np.array_equal(ya0, yb0) and np.array_equal(ya1, yb1)
    # and through the drop-in class: forward at B <= 38, load_state_dict, forward again
    from speech_enhancement_mi_amd import TemporalCRN
    m = TemporalCRN(**FULL512)
    tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
    m.load_state_dict(tsd)
    m = m.cuda()
    y1 = m.realtime_process(_cuda(mix))
    m.load_state_dict(tsd)
    y2 = m.realtime_process(_cuda(mix))
    assert torch.equal(y1, y2) and bool(torch.isfinite(y2).all())


def test_dbg_skip_knob_is_refused_by_the_shipped_library(monkeypatch):
    monkeypatch.setenv("SE_DBG_SKIP", "1")
    with pytest.raises(RuntimeError, match="SE_DEBUG_KNOBS"):
        _engine(TINY)


# ---- the persistent training GRU -----------------------------------------------------------------------------------------------
def _ref_gru_segments(ref, x, h0, seg_len):
    """nn.GRU run segment by segment with a detached carry: exactly what realtime_process does (CRN.py:281, 577-586)."""
    outs, h = [], h0[None]
    T = x.shape[1]
    step = seg_len if seg_len > 0 else T
    for t0 in range(0, T, step):
        o, h = ref(x[:, t0:t0 + step], h.detach() if t0 else h)
        outs.append(o)
    return torch.cat(outs, dim=1), h[0]


@pytest.mark.parametrize("In,H,B,T,seg_len", [(64, 512, 4, 42, 21), (64, 512, 17, 30, 10), (48, 512, 32, 21, 7), (40, 128, 8, 25, 0),
                                              (24, 16, 3, 21, 21), (32, 256, 40, 12, 4), (24, 144, 20, 9, 3)])
def test_persistent_gru_layer_vs_autograd(In, H, B, T, seg_len):
    """gru_layer (k_gru_pseq_fwd / _bwd: register-resident W_hh slices, sc1 state exchange) against nn.GRU + autograd run
    segment by segment: outputs, final state, input gradient and all four parameter gradients.  B = 17..32 takes the two-row-tile
    instances, B = 40 two launches (groups of <= 32 streams), H = 144 the per-step fallback (groups of <= 16: the wide-batch
    route ADVICE r02 asked a test for)."""
    from speech_enhancement_mi_amd import train_ops as K
    torch.manual_seed(H + B)
    ref = torch.nn.GRU(In, H, 1, batch_first=True).cuda()
    x = torch.randn(B, T, In, device="cuda") * 0.5
    h0 = torch.randn(B, H, device="cuda") * 0.5
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ps = [p.detach().clone().requires_grad_(True) for p in (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)]
    out, hT = K.gru_layer(xa, h0, *ps, seg_len=seg_len)
    out_r, hT_r = _ref_gru_segments(ref, xb, h0, seg_len)
    assert _rel(out, out_r) < 1e-5 and _rel(hT, hT_r) < 1e-5
    g = torch.randn_like(out_r)
    gh = torch.randn_like(hT_r)
    (out * g).sum().add((hT * gh).sum()).backward()
    (out_r * g).sum().add((hT_r * gh).sum()).backward()
    K.pseq_check()
    assert _rel(xa.grad, xb.grad) < 2e-5
    for p, q in zip(ps, (ref.weight_ih_l0, ref.weight_hh_l0, ref.bias_ih_l0, ref.bias_hh_l0)):
        assert _rel(p.grad, q.grad) < 1e-4


def test_persistent_gru_is_deterministic_and_batch_independent():
    """Same inputs -> bit-identical outputs across launches (fixed summation order: no atomics in the data path); stream b of
    a 32-stream launch equals the same stream in a 4-stream launch to rounding (different row tile -> same products)."""
    from speech_enhancement_mi_amd import train_ops as K
    torch.manual_seed(3)
    In, H, T = 32, 512, 63
    ps = [torch.randn(3 * H, In, device="cuda") * 0.1, torch.randn(3 * H, H, device="cuda") * 0.05, torch.randn(3 * H, device="cuda") * 0.1,
          torch.randn(3 * H, device="cuda") * 0.1]
    x = torch.randn(32, T, In, device="cuda")
    h0 = torch.randn(32, H, device="cuda") * 0.3
    with torch.no_grad():
        o1, h1 = K.gru_layer(x, h0, *ps)
        o2, h2 = K.gru_layer(x, h0, *ps)
        o4, h4 = K.gru_layer(x[5:9].contiguous(), h0[5:9].contiguous(), *ps)
    K.pseq_check()
    assert torch.equal(o1, o2) and torch.equal(h1, h2)
    assert _rel(o1[5:9], o4) < 1e-6 and _rel(h1[5:9], h4) < 1e-6


# ---- the norm / pointwise / signal kernels of the training step, forward and backward, vs torch autograd --------------------
def _gln_ref(a, w, b):
    dims = tuple(range(1, a.dim()))
    mean = a.mean(dims, keepdim=True)
    var = ((a - mean) ** 2).mean(dims, keepdim=True)
    return (a - mean) / (torch.sqrt(var + 1e-8) + 1e-8) * w + b


@pytest.mark.parametrize("S,C,T,Fi,Fo,act", [(5, 16, 21, 101, 101, 1), (3, 64, 21, 25, 26, 1), (4, 8, 7, 13, 13, 0), (2, 2, 21, 201, 201, 2)])
def test_fused_gln_channel_mode_vs_autograd(S, C, T, Fi, Fo, act):
    """k_tgln_fwd / k_tgln_bwd_c: y = pad(gLN(act(x))) (CRN.py:135-149, 389-392) and its gradients w.r.t. the pre-activation x,
    the affine pair and the producing convolution's bias (= per-channel sum of dx)."""
    from speech_enhancement_mi_amd import train_net as N
    torch.manual_seed(C + Fi)
    x = torch.randn(S, C, T, Fi, device="cuda")
    w, b = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    y = torch.empty(S, C, T, Fo, device="cuda")
    st = N.gln_fwd(x, (C * T * Fi, T * Fi, Fi), N._p(y), (C * T * Fo, T * Fo, Fo), w, b, S, C, T, Fi, Fo, 0, act)
    xr, wr, br = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    actf = {0: lambda v: v, 1: torch.relu, 2: torch.nn.functional.elu}[act]
    yr = torch.nn.functional.pad(_gln_ref(actf(xr), wr.view(1, C, 1, 1), br.view(1, C, 1, 1)), (0, Fo - Fi))
    assert _rel(y, yr) < 1e-5
    gy = torch.randn_like(yr)
    yr.backward(gy)
    dx, dw, db, dpre = N.gln_bwd(N._p(gy), (C * T * Fo, T * Fo, Fo), x, (C * T * Fi, T * Fi, Fi), w, st, S, C, T, Fi, 0, act)
    assert _rel(dx, xr.grad) < 2e-5 and _rel(dw, wr.grad) < 2e-5 and _rel(db, br.grad) < 2e-5
    assert _rel(dpre, xr.grad.sum((0, 2, 3))) < 2e-4


def test_fused_gln_last_mode_vs_autograd():
    """k_tgln_bwd_d: the norm after fc_output_layer (GlobalLayerNorm(last=True), CRN.py:127-129, 274-276): input [S][T][D] rows
    of the dense layer, output re-laid-out to [S][C][T][F], affine per feature d = c * F + f."""
    from speech_enhancement_mi_amd import train_net as N
    torch.manual_seed(9)
    S, C, T, F = 6, 128, 21, 13
    D = C * F
    o = torch.randn(S * T, D, device="cuda")
    w, b = torch.randn(D, device="cuda"), torch.randn(D, device="cuda")
    y = torch.empty(S, C, T, F, device="cuda")
    st = N.gln_fwd(o, (T * D, F, D), N._p(y), (C * T * F, T * F, F), w, b, S, C, T, F, F, 1, 1)
    orr, wr, br = (t.detach().clone().requires_grad_(True) for t in (o, w, b))
    yr = _gln_ref(torch.relu(orr.view(S, 1, T, D)), wr.view(1, 1, 1, D), br.view(1, 1, 1, D)).view(S, T, C, F).permute(0, 2, 1, 3)
    assert _rel(y, yr) < 1e-5
    gy = torch.randn(S, C, T, F, device="cuda")
    yr.backward(gy)
    dx, dw, db, dpre = N.gln_bwd(N._p(gy), (C * T * F, T * F, F), o, (T * D, F, D), w, st, S, C, T, F, 1, 1)
    assert dx.shape == o.shape
    assert _rel(dx, orr.grad) < 2e-5 and _rel(dw, wr.grad) < 2e-5 and _rel(db, br.grad) < 2e-5
    assert _rel(dpre, orr.grad.view(S * T, D).sum(0)) < 2e-4


def test_fused_skip_gate_vs_autograd():
    """k_tskip_fwd / _bwd: out = m * relu(u) + (1 - m) * z, m = sigmoid(gLN(v)) (CRN.py:393-396) with u, v the two halves of the
    stacked 1x1 convolution output."""
    from speech_enhancement_mi_amd import train_ops as K
    torch.manual_seed(4)
    S, Co, T, F = 5, 32, 21, 51
    uv = torch.randn(S, 2 * Co, T, F, device="cuda")
    z = torch.randn(S, Co, T, F, device="cuda")
    nw, nb = torch.randn(Co, device="cuda"), torch.randn(Co, device="cuda")
    out, st = torch.empty_like(z), torch.empty(S, 2, device="cuda")
    lib = K._lib()
    p = lambda t: t.data_ptr()
    K._chk(lib.se_train_skip_fwd(p(uv), p(z), p(nw), p(nb), p(out), p(st), S, Co, T, F, 1, 0, K._st()))
    uvr, zr, nwr, nbr = (t.detach().clone().requires_grad_(True) for t in (uv, z, nw, nb))
    m = torch.sigmoid(_gln_ref(uvr[:, Co:], nwr.view(1, Co, 1, 1), nbr.view(1, Co, 1, 1)))
    outr = m * torch.relu(uvr[:, :Co]) + (1 - m) * zr
    assert _rel(out, outr) < 1e-5
    g = torch.randn_like(outr)
    outr.backward(g)
    duv, dz = torch.empty_like(uv), torch.empty_like(z)
    pw, pb, pbias = torch.empty(S, Co, device="cuda"), torch.empty(S, Co, device="cuda"), torch.empty(S, 2 * Co, device="cuda")
    K._chk(lib.se_train_skip_bwd(p(g), p(uv), p(z), p(nw), p(nb), p(st), p(duv), p(dz), p(pw), p(pb), p(pbias), S, Co, T, F, 1, 0, K._st()))
    assert _rel(duv, uvr.grad) < 2e-5 and _rel(dz, zr.grad) < 2e-5
    assert _rel(pw.sum(0), nwr.grad) < 2e-5 and _rel(pb.sum(0), nbr.grad) < 2e-5
    assert _rel(pbias.sum(0), uvr.grad.sum((0, 2, 3))) < 2e-4


@pytest.mark.parametrize("n_fft,flag", [(400, False), (512, False), (400, True)])
def test_fused_signal_chain_vs_torch_autograd(n_fft, flag):
    """se_sig_stft over all segments == utility.padding/segmentation + torch.stft; mask -> se_sig_istft -> over_add forward against
    torch ops, and the hand-written adjoint chain (over_add^T / envelope -> STFT -> irfft weights -> complex multiply^T ->
    decompress') against torch autograd through torch.istft."""
    import ctypes as C
    from speech_enhancement_mi_amd import train_net as N
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.training import TrainableCRN
    torch.manual_seed(n_fft)
    cfg = dict(TINY, n_fft=n_fft, num_freqs=n_fft // 2 + 1)
    m = TrainableCRN(**cfg).cuda()
    B, M, L = 2, 3, 7000
    Ks, P, T, F = 3200, 1600, 21, n_fft // 2 + 1
    mix, _ = synth.synth_utterances(B, L, M, seed=5)
    x = _cuda(mix)
    lib = K._lib()
    sig = N._sig(x.device, n_fft, 400, 160, Ks)
    Lp = L if flag else L + P
    gap = Ks - (P + Lp % Ks) % Ks
    Nseg = 2 * (Lp + gap + P) // Ks
    S = Nseg * B
    spec = torch.empty(Nseg, B * M, T, F, 2, device="cuda")
    K._chk(lib.se_sig_stft(sig, x.data_ptr(), B, M, L, -P if flag else -2 * P, P, Nseg, spec.data_ptr(), K._st()))
    xt = x if flag else torch.nn.functional.pad(x, (P, 0))
    seg, gap_r = m._segment(xt)                      # [B, M, N, K]
    X = m._stft(seg)                                 # [B, M, N, F, T] complex
    assert gap_r == gap and X.shape[2] == Nseg
    Xr = torch.view_as_real(X.permute(2, 0, 1, 4, 3).contiguous()).reshape(Nseg, B * M, T, F, 2)
    assert _rel(spec, Xr) < 2e-6
    # mask input -> prediction
    xm = (torch.randn(S, 2, T, F, device="cuda") * 4).requires_grad_(True)   # some values beyond the +-9.9 clamp
    Y = torch.empty(S, T, F, 2, device="cuda")
    K._chk(lib.se_train_mask_fwd(xm.data_ptr(), spec.data_ptr(), Y.data_ptr(), S, M, T, F, K._st()))
    yseg = torch.empty(S, Ks, device="cuda")
    K._chk(lib.se_sig_istft(sig, Y.data_ptr(), S, yseg.data_ptr(), K._st()))
    skip = 0 if flag else P
    pred = torch.empty(B, L, device="cuda")
    K._chk(lib.se_train_ola_fwd(sig, yseg.data_ptr(), pred.data_ptr(), B, L, skip, K._st()))
    # torch reference of the same chain
    X0 = X[:, 0].permute(1, 0, 3, 2)                 # [N, B, T, F]
    mm = xm.view(Nseg, B, 2, T, F).clamp(-9.9, 9.9)
    mm = -10.0 * torch.log((10.0 - mm) / (10.0 + mm))
    Yr = torch.complex(mm[:, :, 0] * X0.real - mm[:, :, 1] * X0.imag, mm[:, :, 1] * X0.real + mm[:, :, 0] * X0.imag)
    ysr = m._istft(Yr.permute(1, 0, 3, 2))           # [B, N, K]
    s1 = ysr[:, 0::2].reshape(B, -1)[:, P:]
    s2 = ysr[:, 1::2].reshape(B, -1)[:, :-P]
    outr = ((s1 + s2) / 2)[:, :-gap]
    outr = outr if flag else outr[:, P:]
    assert outr.shape == pred.shape and _rel(pred, outr) < 2e-5
    g = torch.randn_like(outr)
    outr.backward(g)
    gseg = torch.empty(S, Ks, device="cuda")
    K._chk(lib.se_train_ola_bwd(sig, g.data_ptr(), gseg.data_ptr(), B, Nseg, L, skip, K._st()))
    dY = torch.empty(S, T, F, 2, device="cuda")
    K._chk(lib.se_sig_stft(sig, gseg.data_ptr(), S, 1, Ks, 0, 0, 1, dY.data_ptr(), K._st()))
    dxm = torch.empty(S, 2, T, F, device="cuda")
    K._chk(lib.se_train_mask_bwd(dY.data_ptr(), xm.data_ptr(), spec.data_ptr(), dxm.data_ptr(), S, M, T, F, n_fft, K._st()))
    assert _rel(dxm, xm.grad) < 5e-5


def test_fused_conv1x1_and_deterministic_wgrad():
    """kind 3 (1x1 convolution on [S][C][T][F]) forward, its input gradient (transposed weights), the deterministic weight
    gradient, and bit-reproducibility of the deterministic reductions."""
    from speech_enhancement_mi_amd import train_net as N
    torch.manual_seed(2)
    S, Ci, Co, T, F = 7, 32, 64, 21, 51
    x = torch.randn(S, Ci, T, F, device="cuda")
    w = torch.randn(Co, Ci, device="cuda") * 0.2
    b = torch.randn(Co, device="cuda")
    y = torch.empty(S, Co, T, F, device="cuda")
    N.conv_w(3, N._p(x), None, w, Ci, 1, b, y, S, Ci, Co, T, F, F, 0)
    yr = torch.einsum("oc,sctf->sotf", w, x) + b.view(1, Co, 1, 1)
    assert _rel(y, yr) < 1e-5
    g = torch.randn_like(y)
    dx = torch.empty_like(x)
    N.conv_w(3, N._p(g), None, w, 1, Ci, torch.zeros(Ci, device="cuda"), dx, S, Co, Ci, T, F, F, 0)
    assert _rel(dx, torch.einsum("oc,sotf->sctf", w, g)) < 1e-5
    dw1 = N.wgrad(g, x, None, S, Co, Ci, T, F, F, 0, 1).view(Co, Ci)
    dw2 = N.wgrad(g, x, None, S, Co, Ci, T, F, F, 0, 1).view(Co, Ci)
    assert torch.equal(dw1, dw2)
    assert _rel(dw1, torch.einsum("sotf,sctf->oc", g, x)) < 1e-5
    a, bm = torch.randn(3000, 96, device="cuda"), torch.randn(3000, 40, device="cuda")
    t1, t2 = N.gemm_tn(a, bm), N.gemm_tn(a, bm)
    assert torch.equal(t1, t2) and _rel(t1, a.t() @ bm) < 1e-5
    assert _rel(N.colsum_tall(a), a.sum(0)) < 1e-5


@pytest.mark.parametrize("utts,seconds,accum", [(8, 3.0, 2), (32, 0.6, 1)])
def test_fused_train_step_at_bench_shape_vs_torch_autograd(utts, seconds, accum):
    """BASELINE config 4 at the shape bench.py runs (8 x 3 s, full loss, accumulation 2) and at 32 utterances per micro-batch
    (the two-row-tile persistent GRU).  (a) full loss: loss value and flat gradient of the fused kernels against torch autograd
    (fp32) on the same GPU; (b) where the rounding floor of that comparison lies: with a plain MSE loss both fp32 paths are
    compared against torch autograd in FLOAT64 - the fused kernels must be as close to it as torch's own fp32 kernels are;
    (c) the fused step is bit-reproducible (no atomics)."""
    from speech_enhancement_mi_amd.training import FlatBucket, TrainableCRN
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of(FULL400), seed=2).items()}
    mix, clean = synth.synth_utterances(utts, int(seconds * 16000), 3, seed=85)
    x, c = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()

    def hip_stft(seg):
        """The torch-autograd comparator is fed the SAME fp32 spectrum as the kernels (se_sig_stft): the reference's phase feature
        arctan(im / (re + 1e-8)) (CRN.py:464) jumps by pi where re changes sign, and two correct fp32 FFTs (or fp32 vs fp64) land on
        different sides of re = 0 for about one bin in a million (measured: bin 124 of one frame at this shape, re = -1.2e-7 vs
        +2.3e-7 at a frame maximum of 17) - a property of the feature, not of either implementation."""
        from speech_enhancement_mi_amd import train_net as N, train_ops as K
        rows = seg.reshape(-1, seg.shape[-1]).float().contiguous()
        spec = torch.empty(rows.shape[0], 21, 201, 2, device="cuda")
        K._chk(K._lib().se_sig_stft(N._sig(rows.device, 400, 400, 160, 3200), rows.data_ptr(), rows.shape[0], 1, 3200, 0, 0, 1, spec.data_ptr(), K._st()))
        X = torch.view_as_complex(spec).permute(0, 2, 1).reshape(*seg.shape[:-1], 201, 21)
        return X.to(torch.complex128 if seg.dtype == torch.float64 else torch.complex64)

    def run(hip, loss_kind, dtype=torch.float32):
        m = TrainableCRN(**FULL400)
        m.load_state_dict(sd)
        m = m.cuda().to(dtype).use_hip_kernels(hip)
        if not hip:
            m._stft = hip_stft
        bucket = None if dtype != torch.float32 else FlatBucket(list(m.parameters()))
        total = 0.0
        for xm, cm in zip(x.to(dtype).chunk(accum), c.to(dtype).chunk(accum)):
            pred = m.realtime_process_train(xm)
            if loss_kind == "full":
                lens = torch.full((xm.shape[0],), xm.shape[-1], dtype=torch.int64, device="cuda")
                loss = m.compute_loss(cm, pred, lens)[0] / accum
            else:
                loss = ((pred - cm) ** 2).mean() * (100.0 / accum)
            loss.backward()
            total += float(loss.detach())
        flat = bucket.flat if bucket is not None else torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()])
        return total, flat.detach().clone()

    l_t, g_t = run(False, "full")
    l_h, g_h = run(True, "full")
    l_h2, g_h2 = run(True, "full")
    assert abs(l_h - l_t) < 1e-4 * max(1.0, abs(l_t))
    assert _rel(g_h, g_t) < 3e-3, _rel(g_h, g_t)
    assert l_h == l_h2 and torch.equal(g_h, g_h2)
    _, g64 = run(False, "mse", torch.float64)
    _, gt32 = run(False, "mse")
    _, gh32 = run(True, "mse")
    e_t, e_h = _rel(gt32.double(), g64), _rel(gh32.double(), g64)
    print(f"flat-gradient error vs float64 autograd: torch fp32 {e_t:.2e}, fused kernels {e_h:.2e}")
    assert e_h < max(2.0 * e_t, 5e-5), (e_h, e_t)


def test_merged_microbatches_give_the_accumulated_gradient():
    """train_step(accum=2): one shared forward/backward sweep over both micro-batches with the loss formed per micro-batch gives
    the gradient (and the parameters after Adam) of the sequential accumulation loop to fp32 summation order."""
    from speech_enhancement_mi_amd.training import FlatBucket, TrainableCRN, train_step
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of(FULL400), seed=4).items()}
    mix, clean = synth.synth_utterances(4, 9600, 3, seed=87)
    x, c = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
    lens = torch.tensor([9600, 9000, 9600, 7000], device="cuda")
    res = {}
    for merge in (True, False):
        m = TrainableCRN(**FULL400)
        m.load_state_dict(sd)
        m = m.cuda().use_hip_kernels(True)
        bucket = FlatBucket(list(m.parameters()))
        opt = torch.optim.Adam(m.parameters(), lr=3e-4)
        l = train_step(m, bucket, opt, x, c, lens, accum=2, loss="full", merge=merge)
        res[merge] = (l, bucket.flat.clone(), torch.cat([p.detach().flatten() for p in m.parameters()]))
    assert abs(res[True][0] - res[False][0]) < 1e-5 * max(1.0, abs(res[False][0]))
    assert _rel(res[True][1], res[False][1]) < 2e-5
    assert _rel(res[True][2], res[False][2]) < 1e-6


# ---- FullSubNet: bf16x3 mode, train=True single pass, 6-argument compute_loss --------------------------------------------------
def _fsn_model(cfg, precision="fp32"):
    from conftest import fsn_spec
    from speech_enhancement_mi_amd.fullsubnet import FullSubNet
    m = FullSubNet(**cfg)
    sd = synth.make_state_dict(fsn_spec(cfg), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().set_precision(precision)


def test_fsn_bf16x3_mode_vs_reference_goldens(fgolden):
    """fsn_config.precision = 2 (hi*hi + hi*mid + mid*hi in the LSTM step GEMMs) against the outputs of the genuine reference
    FullSubNet at north_star's bar: relative RMS < 1e-4 and SI-SDR within 0.02 dB (full size, tiny + continuation)."""
    from conftest import FSN_FULL, FSN_TINY
    mix, clean = synth.synth_utterances(1, 4800, 3, seed=7)
    y = _fsn_model(FSN_FULL, "bf16x3").realtime_process(torch.from_numpy(mix).cuda(), None, False, False).cpu().numpy()
    ref = fgolden["fsn_full_out"]
    assert rel_rms(y, ref) < 1e-4, rel_rms(y, ref)
    assert np.abs(synth.si_sdr(clean, y) - synth.si_sdr(clean, ref)).max() < 0.02
    mix, _ = synth.synth_utterances(2, 8000 + 4800, 3, seed=7)
    m = _fsn_model(FSN_TINY, "bf16x3")
    x = torch.from_numpy(mix).cuda()
    y1 = m.realtime_process(x[..., :8000].contiguous(), None, False, False).cpu().numpy()
    y2 = m.realtime_process(x[..., 8000:].contiguous(), None, True, False).cpu().numpy()
    assert rel_rms(y1, fgolden["fsn_tiny_out"]) < 1e-4 and rel_rms(y2, fgolden["fsn_tiny_cont_out"]) < 1e-4
    with pytest.raises(ValueError):
        m.set_precision("fp16")


def test_fsn_train_true_single_pass_vs_reference_golden():
    """FullSubNet.realtime_process(train=True) (fullsubnet.py:921-927: one forward over all N*T frames) against the genuine
    reference's 4-tuple (tests/golden/make_golden_fsn_train.py)."""
    import os
    from conftest import FSN_TINY, ROOT
    g = np.load(os.path.join(ROOT, "tests", "golden", "fsn_train_golden.npz"))
    m = _fsn_model(FSN_TINY)
    mix, clean = synth.synth_utterances(2, 8000, 3, seed=7)
    src = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    y, crm, s, x = m.realtime_process(torch.from_numpy(mix).cuda(), src, flag=False, train=True)
    assert rel_rms(y.cpu().numpy(), g["fsn_tiny_train_out"]) < 1e-4
    assert rel_rms(crm[1:3].cpu().numpy(), g["fsn_tiny_train_crm"]) < 1e-4
    assert rel_rms(s[1:2].cpu().numpy(), g["fsn_tiny_train_s"]) < 1e-5 and rel_rms(x[1:2].cpu().numpy(), g["fsn_tiny_train_x"]) < 1e-5
    # train=False differs (one norm update and one LSTM seam per window): the two paths are not interchangeable
    y_stream = m.realtime_process(torch.from_numpy(mix).cuda(), src, flag=False, train=False)[0]
    assert rel_rms(y_stream.cpu().numpy(), g["fsn_tiny_train_out"]) > 1e-3
    with pytest.raises(NotImplementedError):
        m.realtime_process(torch.from_numpy(mix).cuda(), src, flag=True, train=True)


def test_fsn_compute_loss_six_arguments():
    """FullSubNet.compute_loss(source, pred_source, xf, sf, cIRM, length) (fullsubnet.py:964-986) = the CRN loss on (source, pred, length)."""
    import os
    import sys
    from conftest import FSN_TINY, ROOT
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from loss_inputs import make_loss_inputs
    lg = np.load(os.path.join(ROOT, "tests", "golden", "loss_golden.npz"))
    clean, pred, lens = make_loss_inputs()
    m = _fsn_model(FSN_TINY)
    loss, stoi, sisnr = m.compute_loss(_cuda(clean), _cuda(pred), None, None, None, torch.from_numpy(lens).cuda())
    got = np.array([float(loss), float(stoi), float(sisnr)])
    assert np.abs(got - lg["loss"]).max() < 1e-4, got


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_fsn_big_tile_lstm_step_equals_128_tiles(prec, monkeypatch):
    """k_lstm_step_big (256 rows x 64 units per workgroup, picked for the sub-band model from B*F >= 8192 rows) accumulates every
    element over the same chunks, planes and term order as k_lstm_step_x6's 128 x 128 tiles: same output to rounding at B = 40
    (R = 40 * 257 = 10 280: 41 row blocks, the last one ragged), and the batch-2 prefix equals a B = 2 run on the small tiles."""
    from conftest import FSN_FULL
    mix, _ = synth.synth_utterances(40, 6400, 3, seed=19)
    x = torch.from_numpy(mix).cuda()
    big = _fsn_model(FSN_FULL, prec).realtime_process(x, None, False, False).cpu().numpy()
    monkeypatch.setenv("SE_FSN_BIG", "0")
    small = _fsn_model(FSN_FULL, prec).realtime_process(x, None, False, False).cpu().numpy()
    monkeypatch.delenv("SE_FSN_BIG")
    assert np.isfinite(big).all() and rel_rms(big, small) < 1e-6, rel_rms(big, small)
    two = _fsn_model(FSN_FULL, prec).realtime_process(x[:2].contiguous(), None, False, False).cpu().numpy()
    assert rel_rms(big[:2], two) < 1e-6


def test_fsn_window_pipeline_is_bit_identical_to_one_stream(monkeypatch):
    """fsn_realtime_process runs the full-band model of window n + 1 on a side stream while the sub-band model of window n runs on the
    caller's stream (events guard mag / fb_out / the two-slot spectrum ring).  Same kernels, same order per buffer: the output, also of a
    flag=True continuation, is bit-identical to SE_FSN_PIPELINE=0."""
    from conftest import FSN_FULL
    mix, _ = synth.synth_utterances(3, 9600 + 6400, 3, seed=29)
    x = torch.from_numpy(mix).cuda()
    outs = []
    for piped in (True, False):
        if not piped:
            monkeypatch.setenv("SE_FSN_PIPELINE", "0")
        m = _fsn_model(FSN_FULL)
        y1 = m.realtime_process(x[..., :9600].contiguous(), None, False, False).cpu().numpy()
        y2 = m.realtime_process(x[..., 9600:].contiguous(), None, True, False).cpu().numpy()
        outs.append((y1, y2))
    monkeypatch.delenv("SE_FSN_PIPELINE")
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("precision", [0, 2, 1])
def test_student_feature_taps_device_form_equals_host_form(precision):
    """se_read_tap_dev("ft<k>") (the k_conv_p re-run on the planes in the ring slot, one device transposition k_tap_r_to_bcft) writes
    exactly what the host tap returns (the same two launches and a copy), at the full student geometry and in every operand format
    (3 / 2 bf16 planes, one fp16 plane)."""
    e = _engine(STUDENT400, variant=2, precision=precision, seed=1)
    mix, _ = synth.synth_utterances(3, 6400, 3, seed=31)
    e.reset(3)
    for n in range(2):
        e.step(_cuda(mix[:, :, n * 1600:n * 1600 + 3200]))
    for k in range(5):
        host = e.read_tap(f"ft{k}")
        dev = e.read_tap_dev(f"ft{k}", host.size)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host), k
    with pytest.raises(RuntimeError):
        e.read_tap_dev("enc0", 16)


def test_stoi_kernels_equal_the_torch_restatement():
    """csrc/se_stoi.hip (6 launches forward, 4 backward) against losses._stoi_d (the batched torch restatement that is pinned to the genuine
    reference by loss_golden.npz): per-utterance STOI and the gradient w.r.t. the prediction, full-length and ragged utterances incl. one
    with fewer than 30 spectrogram frames (utility.py:882-885) and one too short to score (0.99, utility.py:877-880).

    Values agree to fp32 spectra (a direct DFT here, rocFFT there).  The GRADIENT of STOI is not continuous - min(alpha Y, (1 + c) X) clips
    10-28 % of the envelope entries and an entry within rounding of the clip edge takes the other branch - so two correct implementations
    differ by ~1e-3 in norm; the correlation stage's backward is therefore also checked exactly, against float64 autograd on the kernels'
    OWN envelopes (2.5e-8), and the linear stages behind it (envelope -> frames -> 10 kHz -> 16 kHz) by the overall agreement."""
    from speech_enhancement_mi_amd import losses
    L = 24000
    mix, clean = synth.synth_utterances(6, L, 3, seed=41)
    src = torch.from_numpy(clean).cuda()
    noise = torch.from_numpy(mix[:, 0].copy()).cuda()
    lens = torch.tensor([24000, 17001, 9000, 20000, 5500, 700], dtype=torch.int64, device="cuda")
    res = []
    for kern in (False, True):
        losses.STOI_KERNELS = kern
        try:
            pred = (0.55 * src + 0.45 * noise).requires_grad_()
            per = losses.stoi_loss(src, pred, lens, reduction="none")          # -D per utterance
            (per * torch.arange(1, 7, device="cuda")).sum().backward()        # distinct upstream gradients
            res.append((per.detach().cpu().double().numpy(), pred.grad.detach().cpu().double()))
        finally:
            losses.STOI_KERNELS = True
    assert np.abs(res[0][0] - res[1][0]).max() < 5e-5, (res[0][0], res[1][0])
    assert abs(res[1][0][5] + 0.99) < 1e-6
    for b in range(6):
        ref, got = res[0][1][b], res[1][1][b]
        assert float((got - ref).norm() / (ref.norm() + 1e-30)) < 5e-3 or float(ref.norm()) == 0.0, b
        if int(lens[b]) < L:
            assert float(got[int(lens[b]):].abs().max()) == 0.0
    # the correlation stage's backward, exactly: float64 autograd on the envelopes the kernels computed
    pred = (0.55 * src + 0.45 * noise).requires_grad_()
    Dk = losses._StoiHip.apply(src, pred, lens)
    fn = Dk.grad_fn
    (-Dk).sum().backward(retain_graph=True)
    v = losses._stoi_ws_views(fn.saved_tensors[1], 6, L)
    nk = v["nk"].cpu().numpy()
    Ot, Op = v["Ot"].cpu().double(), v["Op"].cpu().double().requires_grad_()
    tot = 0
    for b in range(5):
        T = int(nk[b]) + 2
        X, Y = (Ot[b, :T].unfold(0, 30, 1), Op[b, :T].unfold(0, 30, 1)) if T >= 30 else (Ot[b, :T].T, Op[b, :T].T)
        alpha = X.norm(dim=-1, keepdim=True) / (Y.norm(dim=-1, keepdim=True) + losses.SMALL)
        yc = torch.minimum(Y * alpha, X + X * 5.62341325)
        xn = X - X.mean(-1, keepdim=True)
        xn = xn / (xn.norm(dim=-1, keepdim=True) + losses.SMALL)
        yn = yc - yc.mean(-1, keepdim=True)
        yn = yn / (yn.norm(dim=-1, keepdim=True) + losses.SMALL)
        tot = tot - (xn * yn).sum() / (15.0 * (T - 29) if T >= 30 else 15.0)
    tot.backward()
    got, ref = v["dOp"].cpu().double()[:5], Op.grad[:5]
    assert float((got - ref).norm() / ref.norm()) < 1e-6


# ---- config 5 in its named dtype at size; the bounded regression guard of the round-2 fault -------------------------------------
def test_student_batch1024_fp16_named_dtype():
    """BASELINE configs[4] names fp16: precision = 1 (fp16 MFMA operands, fp32 accumulation and storage of the recurrence / norms) at
    B = 1024: finite, bit-repeatable, batch-independent, and within the documented 3e-3 of the fp32-accurate engine (outside
    north_star's 1e-4 bar by design: bf16x3 is the in-bar fast mode, pinned against the reference goldens)."""
    e16, e32 = _engine(STUDENT400, variant=2, precision=1, seed=1), _engine(STUDENT400, variant=2, precision=0, seed=1)
    L = 9600
    base, clean = synth.synth_utterances(4, L, 3, seed=71)
    big = np.ascontiguousarray(np.tile(base, (256, 1, 1)))
    y_big = e16.realtime_process(_cuda(big)).cpu().numpy()
    assert y_big.shape == (1024, L) and np.isfinite(y_big).all()
    y_ref = e32.realtime_process(_cuda(base)).cpu().numpy()
    y_small = e16.realtime_process(_cuda(base)).cpu().numpy()
    for i in (0, 1, 2, 3, 513, 1023):
        # batch independence inside the fp16 mode: a batch of 4 takes the small-batch routes (fp32 skinny GEMMs, two-launch skip gate), which
        # round differently from the fp16-operand plane kernels of the big batch - same function, fp16-sized differences
        assert rel_rms(y_big[i], y_small[i % 4]) < 1e-3, i
        assert rel_rms(y_big[i], y_ref[i % 4]) < 3e-3, i            # the documented distance to the fp32-accurate engine
        assert abs(synth.si_sdr(clean[i % 4], y_big[i]) - synth.si_sdr(clean[i % 4], y_ref[i % 4])) < 0.1
    assert np.array_equal(e16.realtime_process(_cuda(big)).cpu().numpy(), y_big)


def test_stoi_resampler_at_the_shape_of_the_round2_fault():
    """Round 2 saw a GPU memory-access fault inside compute_loss with a [4, 48000] prediction (MIOpen's strided conv1d on a sliced
    view, replaced by unfold + matmul in losses._resample_batch).  One bounded forward + backward at that shape on a SLICED,
    non-contiguous prediction; no repeats."""
    from speech_enhancement_mi_amd import losses
    torch.manual_seed(0)
    big = torch.randn(4, 48000 + 1600, device="cuda", requires_grad=True)
    pred = big[:, 1600:]                      # the training path hands compute_loss exactly such a view (out[:, P:])
    assert not pred.is_contiguous()
    src = torch.randn(4, 48000, device="cuda")
    lens = torch.full((4,), 48000, dtype=torch.int64, device="cuda")
    r, n_out = losses._resample_batch(pred, lens, losses._plan(pred.device))
    assert r.shape[0] == 4 and bool(torch.isfinite(r).all()) and int(n_out[0]) == 30000
    loss = losses.compute_loss(src, pred, lens)[0]
    loss.backward()
    assert bool(torch.isfinite(big.grad).all()) and float(big.grad[:, :1600].abs().max()) == 0.0


# ---- CRN_ELU (the model train.py:16 trains) on the training kernels ---------------------------------------------------------------
def test_fused_pre5_and_gate_ops_vs_autograd():
    """The CRN_ELU deltas as kernels: the 5-channel 5x5 frequency-dilated pre-conv (forward with ELU, input gradient, weight-gradient
    slab; CRN_ELU.py:335-340 with history rows) and the gated 1x1 pair + norm (k_tgate_fwd / _bwd; CRN_ELU.py:240-241)."""
    import torch.nn.functional as Fn
    from speech_enhancement_mi_amd import train_ops as K
    lib = K._lib()
    torch.manual_seed(11)
    S, C, T, F, fd = 4, 5, 21, 201, 2
    x = torch.randn(S, C, T, F, device="cuda", requires_grad=True)
    xp = torch.randn(S, C, T, F, device="cuda")
    w = (torch.randn(C, C, 5, 5, device="cuda") * 0.2).requires_grad_(True)
    b = torch.randn(C, device="cuda", requires_grad=True)
    a = torch.empty(S, C, T, F, device="cuda")
    K._chk(lib.se_train_pre5(0, x.data_ptr(), xp.data_ptr(), w.data_ptr(), b.data_ptr(), None, a.data_ptr(), S, C, T, F, fd, 2, K._st()))
    # reference layout [B, C, F, T]: cat(buffer = last 4 frames of xp, x) -> Conv2d((5,5), dilation (fd,1), padding (2fd,0)) -> ELU
    inp = torch.cat([xp[:, :, -4:].permute(0, 1, 3, 2), x.permute(0, 1, 3, 2)], dim=-1)
    ar = Fn.elu(Fn.conv2d(inp, w, b, padding=(2 * fd, 0), dilation=(fd, 1))).permute(0, 1, 3, 2)
    assert a.shape == ar.shape and _rel(a, ar) < 1e-5
    g = torch.randn(*ar.shape, device="cuda")   # (randn_like would inherit the permuted strides of the reference-layout tensor)
    ar.backward(g)
    dy = g * torch.where(a > 0, torch.ones_like(a), a + 1)          # ELU' from the saved activation
    dx = torch.empty_like(a)
    K._chk(lib.se_train_pre5(1, None, None, w.data_ptr(), None, dy.data_ptr(), dx.data_ptr(), S, C, T, F, fd, 0, K._st()))
    part = torch.empty(S, C * C * 25, device="cuda")
    K._chk(lib.se_train_pre5(2, x.data_ptr(), xp.data_ptr(), w.data_ptr(), None, dy.data_ptr(), part.data_ptr(), S, C, T, F, fd, 0, K._st()))
    assert _rel(dx, x.grad) < 2e-5 and _rel(part.sum(0).view(C, C, 5, 5), w.grad) < 2e-5
    pp = torch.empty(S, C, device="cuda")
    da = g.clone()
    K._chk(lib.se_train_elu_bwd(da.data_ptr(), a.data_ptr(), pp.data_ptr(), S, C, T, F, K._st()))
    assert _rel(da, dy) < 1e-6 and _rel(pp.sum(0), b.grad) < 2e-5
    # gated pair + norm, output written in the GRU layout [S][T][C*F]
    Cg, Fg = 32, 13
    tg = torch.randn(S, 2 * Cg, T, Fg, device="cuda", requires_grad=True)
    nw, nb = torch.randn(Cg, device="cuda", requires_grad=True), torch.randn(Cg, device="cuda", requires_grad=True)
    D = Cg * Fg
    y = torch.empty(S * T, D, device="cuda")
    stt = torch.empty(S, 2, device="cuda")
    K._chk(lib.se_train_gate_fwd(tg.data_ptr(), nw.data_ptr(), nb.data_ptr(), y.data_ptr(), T * D, Fg, D, stt.data_ptr(), S, Cg, T, Fg, 0, K._st()))
    p = tg[:, :Cg] * torch.sigmoid(tg[:, Cg:])
    yr = _gln_ref(p, nw.view(1, Cg, 1, 1), nb.view(1, Cg, 1, 1)).permute(0, 2, 1, 3).reshape(S * T, D)
    assert _rel(y, yr) < 1e-5
    gy = torch.randn_like(yr)
    yr.backward(gy)
    dtg = torch.empty(S, 2 * Cg, T, Fg, device="cuda")
    pw, pb, pbias = torch.empty(S, Cg, device="cuda"), torch.empty(S, Cg, device="cuda"), torch.empty(S, 2 * Cg, device="cuda")
    K._chk(lib.se_train_gate_bwd(gy.data_ptr(), T * D, Fg, D, tg.data_ptr(), nw.data_ptr(), stt.data_ptr(), dtg.data_ptr(), pw.data_ptr(), pb.data_ptr(),
                                 pbias.data_ptr(), S, Cg, T, Fg, 0, K._st()))
    assert _rel(dtg, tg.grad) < 2e-5 and _rel(pw.sum(0), nw.grad) < 2e-5 and _rel(pb.sum(0), nb.grad) < 2e-5
    assert _rel(pbias.sum(0), tg.grad.sum((0, 2, 3))) < 2e-4


@pytest.mark.parametrize("cfgname,utts,seconds", [("tiny", 2, 0.5), ("full400", 4, 1.0)])
def test_fused_crn_elu_train_step_vs_float64_autograd(cfgname, utts, seconds):
    """CRN_ELU (variant 1) on the training kernels: prediction, continuation and the whole flat gradient against torch autograd in
    float64 (fed the same fp32 spectrum: atan2 phase jumps at re = -0), next to torch's own fp32 kernels."""
    from speech_enhancement_mi_amd import train_net as N, train_ops as K
    from speech_enhancement_mi_amd.training import TrainableCRNELU
    cfg = TINY if cfgname == "tiny" else FULL400
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of_variant(cfg, 1), seed=3).items()}
    L = int(seconds * 16000)
    mix, clean = synth.synth_utterances(utts, L + 4800, 3, seed=91)
    x, c = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()

    def hip_stft(seg):
        rows = seg.reshape(-1, seg.shape[-1]).float().contiguous()
        spec = torch.empty(rows.shape[0], 21, 201, 2, device="cuda")
        K._chk(K._lib().se_sig_stft(N._sig(rows.device, 400, 400, 160, 3200), rows.data_ptr(), rows.shape[0], 1, 3200, 0, 0, 1, spec.data_ptr(), K._st()))
        X = torch.view_as_complex(spec).permute(0, 2, 1).reshape(*seg.shape[:-1], 201, 21)
        return X.to(torch.complex128 if seg.dtype == torch.float64 else torch.complex64)

    def run(hip, dtype):
        m = TrainableCRNELU(**cfg)
        m.load_state_dict(sd)
        m = m.cuda().to(dtype).use_hip_kernels(hip)
        if not hip:
            m._stft = hip_stft
        y1 = m.realtime_process_train(x[..., :L].contiguous().to(dtype))
        y2 = m.realtime_process_train(x[..., L:].contiguous().to(dtype), flag=True)
        loss = ((y1 - c[:, :L].to(dtype)) ** 2).mean() * 100 + ((y2 - c[:, L:].to(dtype)) ** 2).mean() * 100
        loss.backward()
        g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()])
        return y1.detach().double(), y2.detach().double(), g.double()

    r64, r32, rh = run(False, torch.float64), run(False, torch.float32), run(True, torch.float32)
    assert _rel(rh[0], r64[0]) < 2e-5 and _rel(rh[1], r64[1]) < 2e-5
    e_t, e_h = _rel(r32[2], r64[2]), _rel(rh[2], r64[2])
    print(f"CRN_ELU flat-gradient error vs float64 autograd: torch fp32 {e_t:.2e}, training kernels {e_h:.2e}")
    assert e_h < max(3.0 * e_t, 1e-4), (e_h, e_t)


def test_ragged_batch_equals_each_stream_alone():
    """se_realtime_process_ragged: utterances of 1 .. 3.75 s in one zero-padded batch (data_c.py:155-173) - every stream gets the output it
    would get alone (its own utility.padding zeros), and zeros beyond its length."""
    e, e1 = _engine(FULL400, seed=4), _engine(FULL400, seed=4)
    lens = [16000, 41234, 60000, 23999, 1, 3200]
    Lmax = max(lens)
    mix, _ = synth.synth_utterances(len(lens), Lmax, 3, seed=33)
    for b, l in enumerate(lens):
        mix[b, :, l:] = 7.0          # garbage beyond the stream's length must not be read
    y = e.realtime_process(_cuda(mix), lengths=lens).cpu().numpy()
    for b, l in enumerate(lens):
        alone = e1.realtime_process(_cuda(mix[b:b + 1, :, :l])).cpu().numpy()
        assert rel_rms(y[b, :l], alone[0]) < 2e-6 or l == 1, (b, l)
        assert np.all(y[b, l:] == 0.0)
    with pytest.raises(RuntimeError, match="outside"):
        e.realtime_process(_cuda(mix), lengths=[Lmax + 1] * len(lens))


def test_ragged_batch_prefix_compaction_is_exact_and_saves_work():
    """At a batch on the plane-GEMM route (48 streams) the shim sorts a ragged batch by length and the engine launches every segment for
    the prefix of streams still running only (se_engine::Bact): each stream still gets exactly the output it gets alone - in the caller's
    original order - and a batch whose streams are short except one costs a fraction of the full-length batch."""
    import time
    B = 48
    e, e1 = _engine(FULL400, seed=4), _engine(FULL400, seed=4)
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(16000, 60001, B)]
    lens[7], lens[20], lens[33] = 60000, 16000, 16000
    Lmax = max(lens)
    mix, _ = synth.synth_utterances(B, Lmax, 3, seed=35)
    for b, l in enumerate(lens):
        mix[b, :, l:] = -3.0
    x = _cuda(mix)
    y = e.realtime_process(x, lengths=lens).cpu().numpy()
    for b in (0, 7, 13, 20, 33, 47):
        l = lens[b]
        alone = e1.realtime_process(_cuda(mix[b:b + 1, :, :l])).cpu().numpy()
        assert rel_rms(y[b, :l], alone[0]) < 2e-6, (b, l)
        assert np.all(y[b, l:] == 0.0)
    # an already sorted batch given as a continuation-free call, and the same batch unsorted: identical per stream
    order = sorted(range(B), key=lambda i: -lens[i])
    ys = e.realtime_process(_cuda(mix[order]), lengths=[lens[i] for i in order]).cpu().numpy()
    assert np.array_equal(ys, y[order])

    # the saving shows where segments are throughput-bound: 256 streams, all but one a third as long as the longest (the 21 segments the
    # one long stream runs alone are latency-bound, ~1 ms each on tilings chosen for 256 streams: 0.74 of the full batch's time measured)
    Bb, Lb = 256, 48000
    xb = torch.randn(Bb, 3, Lb, device="cuda") * 0.1

    def timed(ln):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            e.realtime_process(xb, lengths=ln)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    short = [16000] * Bb
    short[5] = Lb
    timed(short)
    t_short, t_full = timed(short), timed([Lb] * Bb)
    assert t_short < 0.95 * t_full, (t_short, t_full)  # 1.0 without compaction; generous because it is a clock
