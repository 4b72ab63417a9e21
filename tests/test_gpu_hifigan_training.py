"""GPU tests of the HiFi-GAN generator's training path (hifigan_training.HifiFunction, csrc/se_hifi_train.hip): the new kernels against
float64 torch autograd of the restatement's own formulas at the smallest shapes that can still go wrong (1e-5 relative RMS, as
test_gpu_hifigan.py asks of the forward kernels), then the whole node against the genuine reference's gradient fixture
(tests/golden/make_golden_hifigan_grad.py; outputs 1e-4, gradients 1e-3: test_gpu_gbf_training.py's bounds), the forward's bit-equality
with the inference path, reproducibility, the FULL geometry against the float64 restatement, and Hifi_GAN.train_stage."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.hifigan import Generator, Hifi_GAN
from speech_enhancement_mi_amd.train_net import _p

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402
import make_golden_hifigan_grad as mgr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_model(cfg, dtype=torch.float32):
    m = Generator(**cfg).eval()
    m.load_state_dict(mh.state_dict(cfg), strict=True)
    return m.to(DEV).to(dtype)


def rng(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape) * scale)


def dev(t):
    return t.detach().float().to(DEV).contiguous()


def new(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def err(got, want):
    return rel_rms(got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy())


def gate(y):
    return torch.tanh(y) * torch.sigmoid(y)


# ---- the kernels against float64 torch autograd ------------------------------------------------------------------------------------
def test_lstm_training_kernels():
    """11 utterances x 2 windows of 5 steps: the forward's tile of 8 rows has a tail of 3, the backward's 22 rows one of 6; (h0, c0)
    non-zero, so the first window's c_{t-1} and h_{t-1} come from the entry state and the second's from the row before."""
    lib = K._lib()
    B, Nc, T, H = 11, 2, 5, 24
    TT = Nc * T
    gi = rng(1, B, TT, 4 * H).requires_grad_(True)
    whh = rng(2, 4 * H, H, scale=0.3).requires_grad_(True)
    h0, c0, R = rng(3, B, H, scale=0.5), rng(4, B, H, scale=0.5), rng(5, B, TT, H)
    h, c, outs = h0, c0, []
    for t in range(TT):
        if t % T == 0:
            h, c = h.detach(), c.detach()   # the window seam
        g = gi[:, t] + h @ whh.t()
        c = torch.sigmoid(g[:, H:2 * H]) * c + torch.sigmoid(g[:, :H]) * torch.tanh(g[:, 2 * H:3 * H])
        h = torch.sigmoid(g[:, 3 * H:]) * torch.tanh(c)
        outs.append(h)
    want_out = torch.stack(outs, dim=1)
    want_dgi, want_dw = torch.autograd.grad((want_out * R).sum(), [gi, whh])

    gid, whd, h0d, c0d = dev(gi), dev(whh), dev(h0), dev(c0)
    plain = [new(B * TT, H), new(B, H), new(B, H)]
    K._chk(lib.se_hifi_lstm(_p(gid), _p(h0d), _p(c0d), _p(whd), *[_p(t) for t in plain], B, TT, H, K._st()))
    train = [new(B * TT, H), new(B, H), new(B, H)]
    gates, cs = new(B * TT, 4 * H), new(B * TT, H)
    K._chk(lib.se_hifi_lstm_train_fwd(_p(gid), _p(h0d), _p(c0d), _p(whd), *[_p(t) for t in train], _p(gates), _p(cs), B, TT, H, K._st()))
    for a, b in zip(plain, train):
        assert torch.equal(a, b)
    assert err(train[0].view(B, TT, H), want_out) <= 1e-5 and torch.equal(cs.view(B, TT, H)[:, -1], train[2])
    dg, dc, Rd, wt = new(B * TT, 4 * H), new(B * Nc, H), dev(R), whd.t().contiguous()   # named: a temporary's memory is reused at once
    hp, cp = new(B * TT, H), new(B * TT, H)
    K._chk(lib.se_train_gru_hprev(_p(train[0]), _p(h0d), _p(hp), B, TT, H, TT, 0, TT, K._st()))
    K._chk(lib.se_train_gru_hprev(_p(cs), _p(c0d), _p(cp), B, TT, H, TT, 0, TT, K._st()))
    K._chk(lib.se_hifi_lstm_bwd(_p(Rd), _p(gates), _p(cs), _p(cp), _p(wt), _p(dg), _p(dc), B, Nc, T, H, K._st()))
    e_gi, e_w = err(dg.view(B, TT, 4 * H), want_dgi), err(K.gemm_tn(dg, hp), want_dw)
    print(f"lstm backward: dgi {e_gi:.2e}, dW_hh {e_w:.2e}")
    assert e_gi <= 1e-5 and e_w <= 1e-5


@pytest.mark.parametrize("step0", [0, 40])
def test_seqnorm_backward_kernel(step0):
    """once from nothing carried (the first window is normalised by its own mean: alpha = 0) and once from a carried mean at step 40"""
    lib = K._lib()
    B, Nc, C_, T, F = 2, 3, 2, 3, 5
    D, S = C_ * F, Nc * B
    o = rng(6, B, Nc, T, D).requires_grad_(True)
    w, bias = (1.0 + rng(7, D, scale=0.3)).requires_grad_(True), rng(8, D, scale=0.3).requires_grad_(True)
    mean_in = rng(9, B, scale=0.2) if step0 else torch.zeros(B, dtype=torch.float64)
    dy = rng(10, S, C_, T, F)
    th = torch.tanh(o)
    gm, step, ys = mean_in, float(step0), []
    for n in range(Nc):
        alpha = step / (step + D)
        cur = alpha * gm + (1.0 - alpha) * th[:, n].mean(dim=(1, 2))
        ys.append((th[:, n] - cur[:, None, None]) * w + bias)
        gm, step = cur.detach(), step + D
    y = torch.stack(ys, dim=0).reshape(S, T, C_, F).transpose(1, 2)     # [S = n B + b][C][T][F]
    want = torch.autograd.grad((y * dy).sum(), [o, w, bias])

    od, wd, bd, md, dyd = dev(o), dev(w), dev(bias), dev(mean_in), dev(dy)
    wm, mean_out, yk = new(B * Nc), new(B), new(S, C_, T, F)
    K._chk(lib.se_hifi_seqnorm(_p(od), _p(wd), _p(bd), _p(md), float(step0), _p(wm), _p(mean_out), _p(yk), Nc, B, C_, T, F, K._st()))
    assert err(yk, y) <= 1e-5
    em, do, pw, pb = new(S), new(B * Nc * T, D), new(S, D), new(S, D)
    K._chk(lib.se_hifi_seqnorm_bwd(_p(dyd), _p(od), _p(wd), _p(wm), float(step0), _p(em), _p(do), _p(pw), _p(pb), Nc, B, C_, T, F, K._st()))
    dw, db = K.colsum3(S, (pw, D), (pb, D))
    es = [err(do.view(B, Nc, T, D), want[0]), err(dw, want[1]), err(db, want[2])]
    print(f"seqnorm backward from step {step0}: do {es[0]:.2e}, dw {es[1]:.2e}, db {es[2]:.2e}")
    assert max(es) <= 1e-5


def test_skip_gate_rows_backward_kernels():
    """25 -> 26 frequencies: the padded column takes part in the skip and gives the transposed convolution no gradient"""
    lib = K._lib()
    S, Co, T, Fy, Fr = 2, 4, 3, 25, 26
    yd, uv, dout = rng(11, S, Co, T, Fy).requires_grad_(True), rng(12, S, 2 * Co, T, Fr).requires_grad_(True), rng(13, S, Co, T, Fr)
    z = torch.nn.functional.pad(gate(yd), (0, Fr - Fy))
    m = torch.sigmoid(uv[:, Co:])
    out = m * torch.tanh(uv[:, :Co]) + (1.0 - m) * z
    want = torch.autograd.grad((out * dout).sum(), [uv, yd])
    duv, dyd, ins = new(S, 2 * Co, T, Fr), new(S, Co, T, Fy), [dev(dout), dev(yd), dev(uv)]
    K._chk(lib.se_hifi_skip_bwd(*[_p(t) for t in ins], _p(duv), _p(dyd), S, Co, T, Fy, Fr, K._st()))
    assert err(duv, want[0]) <= 1e-5 and err(dyd, want[1]) <= 1e-5
    # the self-gate's derivative over its whole range
    x = torch.linspace(-12.0, 12.0, 1000, dtype=torch.float64).requires_grad_(True)
    dy = rng(14, 1000)
    want_dx, = torch.autograd.grad((gate(x) * dy).sum(), [x])
    dx, ins = new(1000), [dev(dy), dev(x)]
    K._chk(lib.se_hifi_gate_bwd(*[_p(t) for t in ins], _p(dx), 1000, K._st()))
    assert err(dx, want_dx) <= 1e-5
    # rows adjoint = the inverse permutation, and the channel sums
    Nc, B, C_, F = 2, 3, 2, 5
    xs = dev(rng(15, Nc * B, C_, T, F))
    rows, back = new(B * Nc * T, C_ * F), new(Nc * B, C_, T, F)
    K._chk(lib.se_hifi_rows(_p(xs), _p(rows), Nc, B, C_, T, F, K._st()))
    K._chk(lib.se_hifi_rows_bwd(_p(rows), _p(back), Nc, B, C_, T, F, K._st()))
    assert torch.equal(back, xs)
    part = new(Nc * B, C_)
    K._chk(lib.se_hifi_chansum(_p(xs), _p(part), Nc * B * C_, T * F, K._st()))
    assert err(part, xs.double().sum(dim=(2, 3))) <= 1e-6


# ---- the whole node ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gg():
    return np.load(os.path.join(ROOT, "tests", "golden", "hifigan_grad_golden.npz"))


def fixture_call(m, gg, c, mix):
    a, b, reset = mgr.CALLS[c]
    m.zero_grad(set_to_none=True)
    pred, before = m.realtime_process(mix[..., a:b].contiguous(), reset=reset)
    ((pred * torch.from_numpy(gg[f"c{c}_R"]).float().to(DEV)).sum() + (before * torch.from_numpy(gg[f"c{c}_Rb"]).float().to(DEV)).sum()).backward()
    return pred, before


def test_training_node_matches_the_reference_fixture(gg):
    """TINY, B = 2, max_segments = 2: call 0 has 6 windows = 3 passes, call 1 continues the carried state"""
    m = make_model(mh.TINY).use_hip_training(True)
    m.max_segments = 2
    mix = torch.from_numpy(mh.mixture()).to(DEV)
    names = [n for n, _ in m.named_parameters()]
    for c in range(len(mgr.CALLS)):
        pred, before = fixture_call(m, gg, c, mix)
        assert m._last_path == "kernel" and pred.grad_fn is before.grad_fn and "HifiFunction" in type(pred.grad_fn).__name__
        if c == 0:
            assert m._last_passes == [(0, 2, 2), (2, 2, 2), (4, 2, 2)]
        e_out = max(err(pred, torch.from_numpy(gg[f"c{c}_pred"])), err(before, torch.from_numpy(gg[f"c{c}_before"])))
        worst, who = 0.0, None
        for n, p in m.named_parameters():
            ref = gg[f"c{c}_g_{n}"]
            if not np.any(ref):
                assert p.grad is None, n
                continue
            e = rel_rms(mgr.stored(c, n, p.grad.cpu().numpy()), ref)
            worst, who = (e, n) if e > worst else (worst, who)
        print(f"call {c}: outputs {e_out:.2e}, worst gradient {worst:.2e} ({who})")
        assert e_out <= 1e-4 and worst <= 1e-3, (c, who)
    assert len(names) == len(set(names))


def test_training_forward_is_the_inference_path_bit_for_bit():
    mix = torch.from_numpy(mh.mixture()).to(DEV)
    chunks = [(0, 3200, True), (3200, 6400, False), (6400, 8000, False)]

    def session(train_second):
        m = make_model(mh.TINY)
        m.max_segments = 2
        outs = []
        for i, (a, b, reset) in enumerate(chunks):
            x = mix[..., a:b].contiguous()
            if i == 1 and train_second:
                m.use_hip_training(True)
                pred, before = m.realtime_process(x, reset=reset)
                assert pred.requires_grad and m._last_path == "kernel"
                (pred.sum() + before.sum()).backward()
                m.use_hip_training(False)
            else:
                with torch.no_grad():
                    pred, before = m.realtime_process(x, reset=reset)
            state = [t.clone() for k in ("buf", "h", "c") for t in m._kstate[k]] + [m._nstate["mean"].clone()]
            outs.append((pred.detach(), before.detach(), state, m._nstate["step"]))
        return outs

    for (p0, b0, s0, n0), (p1, b1, s1, n1) in zip(session(False), session(True)):
        assert torch.equal(p0, p1) and torch.equal(b0, b1) and n0 == n1
        assert len(s0) == len(s1) and all(torch.equal(x, y) for x, y in zip(s0, s1))


def test_training_gradients_are_reproducible(gg):
    mix = torch.from_numpy(mh.mixture()).to(DEV)
    runs = []
    for _ in range(2):
        m = make_model(mh.TINY).use_hip_training(True)
        m.max_segments = 2
        fixture_call(m, gg, 0, mix)
        runs.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert runs[0].keys() == runs[1].keys() and all(torch.equal(runs[0][n], runs[1][n]) for n in runs[0])


def test_training_refuses_chains_and_per_stream_steps():
    m = make_model(mh.TINY).use_hip_training(True)
    mix = torch.from_numpy(mh.mixture()).to(DEV)[..., :4800].contiguous()
    with pytest.raises(ValueError, match=r"use_hip_training\(False\)"):
        m.realtime_process_chains(mix, [True, True], [4800, 3200])
    with torch.no_grad():
        m.realtime_process_chains(mix, [True, True], [4800, 1600])   # the streams' norm step counts now differ
    assert isinstance(m._nstate["step"], list)
    with pytest.raises(ValueError, match=r"use_hip_training\(False\)"):
        m.realtime_process(mix, reset=True)


def test_full_geometry_against_the_float64_restatement():
    mix = torch.from_numpy(mh.mixture()).to(DEV)[:1, :, :4800].contiguous()
    R, Rb = (rng(s, 1, 4800).float().to(DEV) for s in (21, 22))
    m = make_model(mh.FULL).use_hip_training(True)
    pred, before = m.realtime_process(mix, reset=True)
    ((pred * R).sum() + (before * Rb).sum()).backward()
    ref = make_model(mh.FULL, torch.float64)
    p64, b64 = ref.realtime_process(mix.double(), reset=True)
    ((p64 * R.double()).sum() + (b64 * Rb.double()).sum()).backward()
    assert ref._last_path == "torch" and m._last_path == "kernel"
    assert err(pred, p64) <= 1e-4 and err(before, b64) <= 1e-4
    worst, who = 0.0, None
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        unused = n.startswith(("deconvlist.3.residual.", "deconvlist.3.residualmask."))
        assert (p.grad is None) == unused and (q.grad is None) == unused, n
        if not unused:
            e = err(p.grad, q.grad)
            worst, who = (e, n) if e > worst else (worst, who)
    print(f"full geometry: worst gradient rel rms {worst:.2e} ({who})")
    assert worst <= 1e-3, who


def test_train_stage_on_the_kernels():
    mix = torch.from_numpy(mh.mixture()).to(DEV)[..., :4800].contiguous()
    y = torch.from_numpy(mgr.target()).to(DEV)

    def wrapper():
        w = Hifi_GAN([], [], **mh.TINY).eval()
        w.generator.load_state_dict(mh.state_dict(mh.TINY), strict=True)
        return w.to(DEV)

    ref = wrapper()
    want = float(ref.train_stage(mix, y, stage=2, reset=True).detach())
    assert ref.generator._last_path == "torch"
    w = wrapper()
    w.generator.use_hip_training(True)
    opt = torch.optim.Adam(w.parameters(), lr=1e-4)
    loss = w.train_stage(mix, y, stage=2, reset=True)
    assert w.generator._last_path == "kernel" and abs(float(loss.detach()) - want) <= 1e-4 * abs(want)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in w.named_parameters() if ".3.residual" not in n)
    opt.step()
    w.generator.reset_norm()
    after = float(w.train_stage(mix, y, stage=2, reset=True).detach())
    print(f"train_stage: loss {float(loss.detach()):.6f} (restatement {want:.6f}), after one Adam step {after:.6f}")
    assert after < float(loss.detach())
