"""GPU tests of the GTSA kernel path (gtsa.py, csrc/se_gtsa.hip): every se_gtsa_* kernel against the corresponding stage of the torch
restatement in float64 at the smallest shapes that can still go wrong, then the whole path against the genuine reference's fixture and
against the restatement: continuation, chunking, reproducibility, refusals and a 64-utterance batch.

Stage tolerances (relative RMS against float64; all kernel arithmetic is fp32 with statistics combined in double):
  features   2e-6   one sqrt / atan2 per value
  attention  1e-5   67-term fp32 dot products into scores of magnitude up to ~10, which exp() turns from relative into absolute error
                    (x |score|), then sums over maxlen (50 .. 500) probabilities
  addnorm    2e-6   4221-value statistics in double, one fp32 multiply-add per value
  qkv5       2e-6   5-term dot products
  tail5      1e-5   two 105-value norms around an accumulation over fn_dim (up to 1024) x 5 terms
  out stage  1e-5   8442-value statistics, then -10 log((10 - m) / (10 + m)), whose slope at the clip |m| = 9.9 is 100
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.gtsa import GTSA, _gln
from speech_enhancement_mi_amd.train_net import _p

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_gtsa as mgt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F, Fs, T, M = 201, 208, 21, 3


def make_model(tag, device=DEV, **change):
    cfg = dict(dict(mgt.GEOMS)[tag], **change)
    m = GTSA(**cfg).eval()
    m.load_state_dict(mgt.state_dict(cfg), strict=True)
    return m.to(device)


def rng(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape) * scale)


def dev(t):
    return t.float().to(DEV).contiguous()


def padded(x):
    """[..., F] float64 -> [..., Fs] float32 on the GPU, zeros in the pad"""
    return dev(torch.nn.functional.pad(x, (0, Fs - F)))


# ---- the kernels against the restatement's stages in float64 ------------------------------------------------------------------------
@torch.no_grad()
def test_feat_kernel():
    S = 4
    spec = rng(1, S, M, T, F, 2, scale=3.0)
    spec[1, :, 3] = 0.0            # an all-zero frame of every microphone
    spec[2, :, :5] = 0.0           # the leading zeros of a flag=False call
    sk = spec.clone()
    sk[1, :, 3, ::2, 0] = -0.0     # whichever sign of zero an FFT leaves
    sk[2, 1:, :5, :, 1] = -0.0
    x = torch.full((S, 5, T, Fs), float("nan"), device=DEV)
    sk_d = dev(sk)
    K._chk(K._lib().se_gtsa_feat(_p(sk_d), _p(x), S, M, T, F, Fs, K._st()))
    want = GTSA.features(spec.permute(0, 1, 3, 2, 4)).transpose(-1, -2)    # [S, 5, T, F]
    got = x.cpu().double()
    assert torch.isfinite(got).all() and torch.count_nonzero(got[..., F:]) == 0
    assert rel_rms(got[..., :F].numpy(), want.numpy()) < 2e-6
    assert torch.count_nonzero(got[1, 3:, 3, :F]) == 0 and torch.count_nonzero(got[2, 3:, :5, :F]) == 0   # phase differences of zero frames


def attn_reference(q, kn, vn, kc, vc, delta, T_, maxlen, model_dim):
    """q / kn / vn [Nc, B, U, T, Hh, D], kc / vc [B, U, Hh, maxlen, D] (float64) -> (out like q, tape tails like kc)"""
    Nc, B, U, _, Hh, D = q.shape
    tk = torch.cat([kc, kn.permute(1, 2, 4, 0, 3, 5).reshape(B, U, Hh, Nc * T_, D)], dim=3)
    tv = torch.cat([vc, vn.permute(1, 2, 4, 0, 3, 5).reshape(B, U, Hh, Nc * T_, D)], dim=3)
    i = torch.arange(maxlen - T_, maxlen, dtype=torch.float64)
    j = torch.arange(maxlen, dtype=torch.float64)
    G = torch.exp(-(i[:, None] - j[None, :]) ** 2 / (delta ** 2 + 1e-8))
    out = torch.empty_like(q)
    for n in range(Nc):
        lo = (n + 1) * T_
        s = torch.abs(q[n].permute(0, 1, 3, 2, 4) @ tk[..., lo:lo + maxlen, :].transpose(-1, -2) * G / math.sqrt(model_dim))
        out[n] = (torch.softmax(s, dim=-1) @ tv[..., lo:lo + maxlen, :]).permute(0, 1, 3, 2, 4)
    return out, tk[..., -maxlen:, :], tv[..., -maxlen:, :]


ATTN_CASES = {
    # even shape: 2 utterances x 5 channels x 3 heads of 67; the window crosses the carried / new boundary at row 50 - 21 (n + 1), which
    # is no multiple of the 64-key tile, and at N = 4 spans three windows of new keys
    "even": dict(B=2, U=5, Hh=3, D=67, maxlen=50, Nc=4, carried=0.0, ld=208, delta=6.0),
    "odd": dict(B=2, U=201, Hh=1, D=5, maxlen=50, Nc=4, carried=0.0, ld=16, delta=4.0),
    "maxlen500": dict(B=1, U=2, Hh=3, D=67, maxlen=500, Nc=1, carried=0.0, ld=208, delta=11.0),   # 8 key tiles, 479 zero keys
    "carried": dict(B=2, U=5, Hh=3, D=67, maxlen=50, Nc=2, carried=1.0, ld=208, delta=3.0),
    "odd_carried_maxlen210": dict(B=1, U=7, Hh=1, D=5, maxlen=210, Nc=2, carried=1.0, ld=16, delta=12.0),
}


@pytest.mark.parametrize("case", list(ATTN_CASES))
@torch.no_grad()
def test_attn_kernel(case):
    c = ATTN_CASES[case]
    B, U, Hh, D, maxlen, Nc, ld = (c[k] for k in ("B", "U", "Hh", "D", "maxlen", "Nc", "ld"))
    S, HD = Nc * B, Hh * D
    model_dim = 201 if D == 67 else 5
    q = rng(10, Nc, B, U, T, Hh, D, scale=2.0 if D == 67 else 3.0)
    kn, vn = rng(11, Nc, B, U, T, Hh, D), rng(12, Nc, B, U, T, Hh, D)
    kc, vc = rng(13, B, U, Hh, maxlen, D) * c["carried"], rng(14, B, U, Hh, maxlen, D) * c["carried"]
    qkv = torch.zeros(S, U, T, 3 * ld, dtype=torch.float64)   # q | k | v rows, each of stride ld inside one buffer of stride 3 ld
    for o, t_ in enumerate((q, kn, vn)):
        qkv[..., o * ld:o * ld + HD] = t_.reshape(S, U, T, HD)
    qkv_d, kc_d, vc_d = dev(qkv), dev(kc), dev(vc)
    delta = torch.tensor([c["delta"]], device=DEV)
    ldo = HD + 3
    out = torch.full((S, U, T, ldo), float("nan"), device=DEV)
    ko, vo = torch.full_like(kc_d, float("nan")), torch.full_like(vc_d, float("nan"))
    lib = K._lib()
    K._chk(lib.se_gtsa_attn(_p(qkv_d), _p(qkv_d, ld), _p(qkv_d, 2 * ld), _p(kc_d), _p(vc_d), _p(out), _p(delta), 3 * ld, 3 * ld, ldo, S, B, U, Hh, D, T,
                            maxlen, model_dim, K._st()))
    K._chk(lib.se_gtsa_tape(_p(qkv_d, ld), _p(qkv_d, 2 * ld), _p(kc_d), _p(vc_d), _p(ko), _p(vo), 3 * ld, Nc, B, U, Hh, D, T, maxlen, K._st()))
    # the reference sees what the kernel saw: the float32 inputs
    f32 = lambda t_: t_.float().double()  # noqa: E731
    want, tk, tv = attn_reference(f32(q), f32(kn), f32(vn), f32(kc), f32(vc), c["delta"], T, maxlen, model_dim)
    got = out.cpu().double()
    assert torch.isfinite(got[..., :HD]).all() and torch.isnan(got[..., HD:]).all()    # nothing written beyond the heads
    err = rel_rms(got[..., :HD].numpy(), want.reshape(S, U, T, HD).numpy())
    assert err < 1e-5, (case, err)
    assert torch.equal(ko.cpu().double(), tk) and torch.equal(vo.cpu().double(), tv)   # a copy: exact


@pytest.mark.parametrize("in_place", [False, True])
@torch.no_grad()
def test_addnorm_kernel(in_place):
    nseq = 2 * 5
    a, x = rng(20, nseq, T, F) + 0.5, rng(21, nseq, T, F, scale=2.0) - 1.0
    norm = type("N", (), dict(weight=rng(22, 1, 1, F) * 0.25 + 1.0, bias=rng(23, 1, 1, F) * 0.25))
    xd = padded(x)
    y = xd if in_place else torch.full_like(xd, float("nan"))
    a_d, w_d, b_d = dev(a), dev(norm.weight), dev(norm.bias)   # named: alive until the launch is enqueued
    K._chk(K._lib().se_gtsa_addnorm(_p(a_d), F, _p(xd), _p(y), _p(w_d), _p(b_d), nseq, T, F, Fs, K._st()))
    want = _gln(a.float().double() + x.float().double(), type("N", (), dict(weight=norm.weight.float().double(), bias=norm.bias.float().double())))
    got = y.cpu().double()
    assert torch.isfinite(got).all() and torch.count_nonzero(got[..., F:]) == 0
    assert rel_rms(got[..., :F].numpy(), want.numpy()) < 2e-6


def _layer_double(layer):
    import copy
    return copy.deepcopy(layer).cpu().double()


@pytest.mark.parametrize("tag", ["tiny", "full"])   # fn_dim 32 and 1024
@torch.no_grad()
def test_odd_layer_kernels(tag):
    m = make_model(tag)
    layer = m.layers[1]
    a = layer.attention
    fn = layer.linear_in.weight.shape[0]
    S = 3
    x = rng(30, S, 5, T, F, scale=1.5)
    xd = padded(x)
    lib = K._lib()
    qkv = torch.full((S, F, T, 16), float("nan"), device=DEV)
    K._chk(lib.se_gtsa_qkv5(_p(xd), _p(a.ql.weight), _p(a.ql.bias), _p(a.kl.weight), _p(a.kl.bias), _p(a.vl.weight), _p(a.vl.bias), _p(qkv),
                            S, T, F, Fs, K._st()))
    ld = _layer_double(layer)
    rows = x.float().double().permute(0, 3, 2, 1)                      # [S, F, T, 5]: sequences (s, f)
    want = torch.cat([ld.attention.ql(rows), ld.attention.kl(rows), ld.attention.vl(rows)], dim=-1)
    got = qkv.cpu().double()
    assert torch.isfinite(got).all() and torch.count_nonzero(got[..., 15]) == 0
    assert rel_rms(got[..., :15].numpy(), want.numpy()) < 2e-6
    att = rng(31, S, F, T, 8)
    att_d = dev(att)
    y = torch.full_like(xd, float("nan"))
    K._chk(lib.se_gtsa_tail5(_p(att_d), 8, _p(xd), _p(y), _p(a.linear.weight), _p(a.linear.bias), _p(layer.norm_a.weight), _p(layer.norm_a.bias),
                             _p(layer.linear_in.weight), _p(layer.linear_in.bias), _p(layer.linear_out.weight), _p(layer.linear_out.bias),
                             _p(layer.norm_i.weight), _p(layer.norm_i.bias), S, T, F, Fs, fn, K._st()))
    want = ld.after_attention(ld.attention.linear(att.float().double()[..., :5]), rows).permute(0, 3, 2, 1)   # [S, 5, T, F]
    got = y.cpu().double()
    assert torch.isfinite(got).all() and torch.count_nonzero(got[..., F:]) == 0
    assert rel_rms(got[..., :F].numpy(), want.numpy()) < 1e-5
    for f_ in (0, 63, 64, F - 1):   # both ends of f and the seam between two workgroups
        assert rel_rms(got[..., f_].numpy(), want[..., f_].numpy()) < 1e-5, f_
    yi = xd.clone()                  # in place, as the model runs it
    K._chk(lib.se_gtsa_tail5(_p(att_d), 8, _p(yi), _p(yi), _p(a.linear.weight), _p(a.linear.bias), _p(layer.norm_a.weight), _p(layer.norm_a.bias),
                             _p(layer.linear_in.weight), _p(layer.linear_in.bias), _p(layer.linear_out.weight), _p(layer.linear_out.bias),
                             _p(layer.norm_i.weight), _p(layer.norm_i.bias), S, T, F, Fs, fn, K._st()))
    assert torch.equal(yi, y)


@torch.no_grad()
def test_gather3_kernel():
    B, Nc = 2, 3
    S = B * Nc
    x, buf = rng(40, S, 5, T, Fs).float(), rng(41, B, 5, 2, Fs).float()
    A = torch.full((S * T, 15, Fs), float("nan"), device=DEV)
    x_d, buf_d = x.to(DEV), buf.to(DEV)
    K._chk(K._lib().se_gtsa_gather3(_p(x_d), _p(buf_d), _p(A), S, B, T, Fs, K._st()))
    seq = torch.cat([buf] + [x[n * B:(n + 1) * B] for n in range(Nc)], dim=2)      # [B, 5, 2 + Nc T, Fs]
    want = torch.stack([seq[:, :, k:k + Nc * T] for k in range(3)], dim=1)          # [B, 3, 5, Nc T, Fs]
    want = want.reshape(B, 15, Nc, T, Fs).permute(2, 0, 3, 1, 4).reshape(S * T, 15, Fs)
    assert torch.equal(A.cpu(), want)


@torch.no_grad()
def test_out_kernel():
    S, Co = 3, 2 * F
    g = rng(50, S * T, 2 * Co, scale=2.0)
    nw, nb = rng(51, Co) * 2.0 + 8.0, rng(52, Co)          # a wide affine: many mask values beyond +-9.9
    spec = rng(53, S, M, T, F, 2, scale=3.0)
    Y = torch.full((S, T, F, 2), float("nan"), device=DEV)
    tap = torch.full((S, Co, T), float("nan"), device=DEV)
    g_d, nw_d, nb_d, spec_d = dev(g), dev(nw), dev(nb), dev(spec)
    K._chk(K._lib().se_gtsa_out(_p(g_d), 2 * Co, _p(nw_d), _p(nb_d), _p(spec_d), _p(Y), _p(tap), S, M, T, F, K._st()))
    g64 = g.float().double().reshape(S, T, 2 * Co)
    u = (g64[..., :Co] * torch.sigmoid(g64[..., Co:])).transpose(1, 2)                 # [S, Co, T]
    norm = type("N", (), dict(weight=nw.float().double().reshape(1, Co, 1), bias=nb.float().double().reshape(1, Co, 1)))
    mask = _gln(u, norm)
    assert float((mask.abs() > 9.9).double().mean()) > 0.05
    want = GTSA._mask_apply(mask, spec.float().double()[:, 0].transpose(1, 2))          # [S, F, T, 2]
    assert torch.isfinite(Y).all() and torch.isfinite(tap).all()
    assert rel_rms(tap.cpu().numpy(), mask.numpy()) < 1e-5
    assert rel_rms(Y.cpu().permute(0, 2, 1, 3).numpy(), want.numpy()) < 1e-5


# ---- the whole kernel path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_kernel_path_matches_reference_fixture(tag):
    gg = np.load(os.path.join(ROOT, "tests", "golden", "gtsa_golden.npz"))
    m = make_model(tag)
    mix = mgt.mixture()
    with torch.no_grad():
        for c, (a, b, flag) in enumerate(mgt.CHUNKS):
            y = m.realtime_process(torch.from_numpy(mix[..., a:b].copy()).to(DEV), flag=flag).cpu().numpy()
            assert m._last_path == "kernel"
            err = rel_rms(y, gg[f"{tag}_out{c}"])
            print(f"GTSA kernel path vs reference fixture: {tag} chunk {c} rel rms {err:.3e}")
            assert np.isfinite(y).all() and err <= 1e-4, (tag, c, err)


def kernel_spectrum(m):
    """The restatement's spectrum() on the kernels' STFT, so both sides see the same spectrum (atan2 jumps by 2 pi where im changes
    sign at re < 0)."""
    from speech_enhancement_mi_amd.train_net import _sig

    def spectrum(seg):
        B, Mm, N, Ks = seg.shape
        sig = _sig(seg.device, m._cfg["n_fft"], m._win, m._hop, Ks)
        out = torch.empty(1, B * Mm * N, T, F, 2, device=seg.device)
        K._chk(K._lib().se_sig_stft(sig, _p(seg.contiguous().float()), B * Mm * N, 1, Ks, 0, 0, 1, _p(out), K._st()))
        return out.reshape(B, Mm, N, T, F, 2).permute(0, 1, 2, 4, 3, 5)
    return spectrum


def _kernel_vs_restatement(tag, B, chunks):
    mk, mt = make_model(tag), make_model(tag)
    mt.use_hip_kernels(False)
    mt.spectrum = kernel_spectrum(mt)
    mix, _ = synth.synth_utterances(B, sum(chunks), 3, seed=23)
    a = 0
    with torch.no_grad():
        for c, n in enumerate(chunks):
            x = torch.from_numpy(mix[..., a:a + n].copy()).to(DEV)
            yk = mk.realtime_process(x, flag=c > 0)
            yt = mt.realtime_process(x, flag=c > 0)
            assert mt._last_path == "torch" and mk._last_path == "kernel"
            err = rel_rms(yk.cpu().numpy(), yt.cpu().numpy())
            print(f"GTSA kernel path vs restatement: {tag} B={B} chunk {c} rel rms {err:.3e}")
            assert torch.isfinite(yk).all() and err <= 1e-4, (tag, B, c, err)
            a += n


def test_kernel_path_matches_restatement_b8_3s():
    _kernel_vs_restatement("full", 8, [48000])


def test_flag_true_continuation_matches_restatement():
    _kernel_vs_restatement("full", 2, [11200, 6400, 8000])


def test_chunked_equals_unchunked_and_runs_are_bit_identical():
    m = make_model("full")
    mix = torch.from_numpy(synth.synth_utterances(2, 24000, 3, seed=31)[0]).to(DEV)
    with torch.no_grad():
        m.max_segments = 1000
        y_all = m.realtime_process(mix)
        y_all2 = m.realtime_process(mix)
        m.max_segments = 3
        y_3 = m.realtime_process(mix)
    assert torch.equal(y_all, y_all2)
    assert torch.equal(y_all, y_3)


def test_flag_true_with_another_batch_size_raises():
    m = make_model("tiny")
    mix = torch.from_numpy(synth.synth_utterances(2, 6400, 3, seed=3)[0]).to(DEV)
    with torch.no_grad():
        m.realtime_process(mix)
        with pytest.raises(ValueError, match="batch"):
            m.realtime_process(mix[:1], flag=True)


def test_unsupported_geometry_raises_on_the_gpu():
    m = GTSA(**dict(mgt.TINY, maxlen=10)).eval().to(DEV)
    with torch.no_grad(), pytest.raises(ValueError, match="maxlen = 10"):
        m.realtime_process(torch.zeros(1, 3, 3200, device=DEV))


def test_b64_completes_with_finite_output():
    m = make_model("full")
    mix = torch.from_numpy(synth.synth_utterances(64, 48000, 3, seed=41)[0]).to(DEV)
    with torch.no_grad():
        y = m.realtime_process(mix)
    assert m._last_path == "kernel" and y.shape == (64, 48000) and torch.isfinite(y).all()
