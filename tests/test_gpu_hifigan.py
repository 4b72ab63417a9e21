"""GPU tests of the HiFi-GAN generator's kernel path (hifigan.py, csrc/se_hifi.hip): every se_hifi_* kernel against float64 torch at the
smallest shapes that can still go wrong (1e-5 relative RMS, a tenth of the project's bar: fp32 arithmetic with statistics in double),
then the whole path against the genuine reference's fixture (1e-4, the project's bar) and against the restatement run on the GPU:
the three calls of the fixture (the running mean that survives the reset included), the carried state, passes, reproducibility and
the refusal to continue the other path's state."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.hifigan import Generator, fold_weight_norm
from speech_enhancement_mi_amd.train_net import _p

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_model(tag, device=DEV, **change):
    cfg = dict(dict(mh.GEOMS)[tag], **change)
    m = Generator(**cfg).eval()
    m.load_state_dict(mh.state_dict(cfg), strict=True)
    return m.to(device)


def rng(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape) * scale)


def dev(t):
    return t.float().to(DEV).contiguous()


def gate(y):
    return torch.tanh(y) * torch.sigmoid(y)


# ---- the kernels against float64 torch -------------------------------------------------------------------------------------------
def postnet_reference(m, x):
    """x [S, 2, T, F] float64 through the postnet of m with the folded weights in float64"""
    h = x
    for blk in m.postnet:
        w = fold_weight_norm(blk.conv.weight_g, blk.conv.weight_v).cpu()
        h = gate(torch.nn.functional.conv2d(h, w, blk.conv.bias.detach().double().cpu()))
    return h


@torch.no_grad()
@pytest.mark.parametrize("S,T", [(2, 3), (1, 21)])
def test_postnet_kernel(S, T):
    """603 bins per stream: four full 128-bin tiles and a ragged one, two streams; 4221: the real window.  Weights at the fixture's scale."""
    F = 201
    m = make_model("tiny")
    x = rng(10 + S, S, 2, T, F, scale=0.7)
    xd = dev(x)

    def run():
        y = torch.full((S, 2, T, F), float("nan"), device=DEV)
        K._chk(K._lib().se_hifi_postnet(_p(xd), _p(m._postnet_pack()), _p(y), S, T, F, K._st()))
        return y.cpu().double()

    got = run()
    want = postnet_reference(m, x)
    assert torch.isfinite(got).all()
    e = rel_rms(got.numpy(), want.numpy())
    print(f"postnet S={S} T={T}: rel rms {e:.2e}")
    assert e <= 1e-5
    if S == 2:   # a stream's arithmetic does not depend on S
        y1 = torch.empty(1, 2, T, F, device=DEV)
        K._chk(K._lib().se_hifi_postnet(_p(xd[1:]), _p(m._postnet_pack()), _p(y1), 1, T, F, K._st()))
        assert torch.equal(y1.cpu().double()[0], got[1])
    m.postnet[5].conv.weight_g.zero_()   # an inner layer must matter
    dead = run()
    assert rel_rms(dead.numpy(), got.numpy()) > 1e-3
    assert rel_rms(dead.numpy(), postnet_reference(m, x).numpy()) <= 1e-5


@torch.no_grad()
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [16, 512])
def test_lstm_kernel(B, H):
    In, TT = 24, 5
    torch.manual_seed(H + B)
    ref = torch.nn.LSTM(In, H, 1, batch_first=True).double()
    x, h0, c0 = rng(1, B, TT, In), rng(2, B, H, scale=0.5), rng(3, B, H, scale=0.5)
    want, (hT, cT) = ref(x, (h0[None], c0[None]))
    gi = K._gemm(dev(x.reshape(B * TT, In)), dev(ref.weight_ih_l0), dev(ref.bias_ih_l0 + ref.bias_hh_l0))
    h0d, c0d = dev(h0), dev(c0)
    keep = (h0d.clone(), c0d.clone())
    out, hk, ck = (torch.full(s, float("nan"), device=DEV) for s in ((B * TT, H), (B, H), (B, H)))
    whh = dev(ref.weight_hh_l0)
    K._chk(K._lib().se_hifi_lstm(_p(gi), _p(h0d), _p(c0d), _p(whh), _p(out), _p(hk), _p(ck), B, TT, H, K._st()))
    errs = (rel_rms(out.cpu().double().reshape(B, TT, H).numpy(), want.numpy()), rel_rms(hk.cpu().double().numpy(), hT[0].numpy()),
            rel_rms(ck.cpu().double().numpy(), cT[0].numpy()))
    print(f"lstm B={B} H={H}: rel rms out {errs[0]:.2e} h {errs[1]:.2e} c {errs[2]:.2e}")
    assert max(errs) <= 1e-5
    assert torch.equal(h0d, keep[0]) and torch.equal(c0d, keep[1])   # the state it started from is left alone


@torch.no_grad()
def test_skip_kernel():
    S, Co, T, Fy, Fr = 2, 8, 3, 25, 26
    yd, uv = rng(4, S, Co, T, Fy), rng(5, S, 2 * Co, T, Fr)
    out = torch.full((S, Co, T, Fr), float("nan"), device=DEV)
    ydd, uvd = dev(yd), dev(uv)   # held: a pointer taken from a temporary would outlive its memory
    K._chk(K._lib().se_hifi_skip(_p(ydd), _p(uvd), _p(out), S, Co, T, Fy, Fr, K._st()))
    m = torch.sigmoid(uv[:, Co:])
    want = m * torch.tanh(uv[:, :Co]) + (1.0 - m) * torch.nn.functional.pad(gate(yd), (0, Fr - Fy))
    got = out.cpu().double()
    assert rel_rms(got.numpy(), want.numpy()) <= 1e-5
    assert rel_rms(got[..., Fy:].numpy(), (m * torch.tanh(uv[:, :Co]))[..., Fy:].numpy()) <= 1e-6   # the padded column: the skip alone


@torch.no_grad()
@pytest.mark.parametrize("carried", [False, True])
def test_seqnorm_kernel(carried):
    B, Nc, T, C_, F = 2, 3, 3, 8, 13
    D = C_ * F
    o, w, b = rng(6, B, Nc, T, D, scale=1.5), 1.0 + 0.25 * rng(7, D), 0.25 * rng(8, D)
    mean0, step0 = (rng(9, B, scale=0.1), 5 * D) if carried else (torch.zeros(B, dtype=torch.float64), 0)
    a = torch.tanh(o)
    g, step, gs = mean0.clone(), step0, []
    for n in range(Nc):
        alpha = step / (step + D)
        g = alpha * g + (1.0 - alpha) * a[:, n].mean(dim=(1, 2))
        gs.append(g)
        step += D
    y64 = (a - torch.stack(gs, dim=1)[:, :, None, None]) * w + b                      # [B, Nc, T, D]
    want = y64.reshape(B, Nc, T, C_, F).permute(1, 0, 3, 2, 4).reshape(Nc * B, C_, T, F)
    y, wm, mo = torch.full((Nc * B, C_, T, F), float("nan"), device=DEV), torch.empty(B * Nc, device=DEV), torch.empty(B, device=DEV)
    od, wd, bd, md = dev(o), dev(w), dev(b), dev(mean0)
    K._chk(K._lib().se_hifi_seqnorm(_p(od), _p(wd), _p(bd), _p(md), float(step0), _p(wm), _p(mo), _p(y), Nc, B, C_, T, F, K._st()))
    assert rel_rms(y.cpu().double().numpy(), want.numpy()) <= 1e-5
    assert float((mo.cpu().double() - g).abs().max()) <= 1e-6
    assert float((wm.cpu().double().reshape(B, Nc) - torch.stack(gs, dim=1)).abs().max()) <= 1e-6


@torch.no_grad()
def test_rows_and_gate_kernels():
    Nc, B, C_, T, F = 2, 3, 4, 3, 13
    x = rng(11, Nc * B, C_, T, F)
    xd = dev(x)
    rows = torch.empty(B * Nc * T, C_ * F, device=DEV)
    K._chk(K._lib().se_hifi_rows(_p(xd), _p(rows), Nc, B, C_, T, F, K._st()))
    want = x.float().reshape(Nc, B, C_, T, F).permute(1, 0, 3, 2, 4).reshape(B * Nc * T, C_ * F)
    assert torch.equal(rows.cpu(), want)
    y = torch.empty_like(xd)
    K._chk(K._lib().se_hifi_gate(_p(xd), _p(y), xd.numel(), K._st()))
    assert rel_rms(y.cpu().double().numpy(), gate(x).numpy()) <= 1e-6


# ---- the whole path --------------------------------------------------------------------------------------------------------------
def run_calls(m):
    """the fixture's three calls -> [(pred, pred_before, state, norm state) per call]"""
    mix = mh.mixture()
    out = []
    with torch.no_grad():
        for a, b, reset in mh.CALLS:
            pred, before = m.realtime_process(torch.from_numpy(mix[..., a:b].copy()).to(DEV), reset=reset)
            st = m._kstate if m._last_path == "kernel" else m._tstate
            out.append((pred.cpu(), before.cpu(), st, dict(m._nstate)))
    return out


@pytest.fixture(scope="module", params=["tiny", "full"])
def runs(request):
    tag = request.param
    mk, mt = make_model(tag), make_model(tag).use_hip_kernels(False)
    rk, rt = run_calls(mk), run_calls(mt)
    assert mk._last_path == "kernel" and mt._last_path == "torch"
    return tag, rk, rt


def test_kernel_path_matches_reference_and_restatement(runs):
    tag, rk, rt = runs
    hg = np.load(os.path.join(ROOT, "tests", "golden", "hifigan_golden.npz"))
    for c in range(3):
        for i, name in enumerate(("pred", "before")):
            e_ref, e_t = rel_rms(rk[c][i].numpy(), hg[f"{tag}_c{c}_{name}"]), rel_rms(rk[c][i].numpy(), rt[c][i].numpy())
            print(f"{tag} call {c} {name}: kernel path vs reference {e_ref:.2e}, vs restatement on the GPU {e_t:.2e}")
            assert e_ref <= 1e-4 and e_t <= 1e-4, (tag, c, name, e_ref, e_t)
    assert not torch.equal(rk[0][0], rk[2][0])   # the third call is the first again, but for the running mean


def test_carried_state_matches_the_restatement(runs):
    tag, rk, rt = runs
    hg = np.load(os.path.join(ROOT, "tests", "golden", "hifigan_golden.npz"))
    for c in range(3):
        ks, ts, kn, tn = rk[c][2], rt[c][2], rk[c][3], rt[c][3]
        for kb, tb in zip(ks["buf"], ts["buf"]):     # [B][C][T][F], the whole last window, against [B, C, F, P], its last P frames
            P = tb.shape[-1]
            assert rel_rms(kb[:, :, -P:].transpose(2, 3).cpu().numpy(), tb.cpu().numpy()) <= 1e-5
        for l, (h, cc) in enumerate(ts["hc"]):
            assert rel_rms(ks["h"][l].cpu().numpy(), h.cpu().numpy()) <= 1e-5 and rel_rms(ks["c"][l].cpu().numpy(), cc.cpu().numpy()) <= 1e-5, (tag, c, l)
        assert kn["step"] == tn["step"] == int(hg[f"{tag}_c{c}_step"][0])
        assert float((kn["mean"].cpu() - tn["mean"].cpu()).abs().max()) <= 1e-5
        assert float(np.abs(kn["mean"].cpu().numpy() - hg[f"{tag}_c{c}_mean"]).max()) <= 1e-5


def _same_state(a, b):
    return all(torch.equal(x, y) for k in ("buf", "h", "c") for x, y in zip(a[k], b[k]))


def test_passes_and_reruns_are_bit_identical():
    rk = run_calls(make_model("tiny"))
    one = make_model("tiny")
    one.max_segments = 1
    r1 = run_calls(one)
    r2 = run_calls(make_model("tiny"))
    for c in range(3):
        for r in (r1, r2):
            assert torch.equal(r[c][0], rk[c][0]) and torch.equal(r[c][1], rk[c][1])
            assert _same_state(r[c][2], rk[c][2]) and torch.equal(r[c][3]["mean"], rk[c][3]["mean"]) and r[c][3]["step"] == rk[c][3]["step"]


def test_continuing_the_other_paths_state_is_refused():
    m = make_model("tiny")
    x = torch.from_numpy(mh.mixture()[..., :3200].copy()).to(DEV)
    with torch.no_grad():
        m.use_hip_kernels(False).realtime_process(x, reset=True)
        before = m._tstate
        m.use_hip_kernels(True)
        with pytest.raises(RuntimeError, match="other path"):
            m.realtime_process(x, reset=False)
        assert m._tstate is before and m._kstate is None
        pred, _ = m.realtime_process(x, reset=True)
    assert m._last_path == "kernel" and torch.isfinite(pred).all()
