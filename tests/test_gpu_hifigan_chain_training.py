"""GPU tests of the HiFi-GAN generator's chunk-chain training (`use_hip_training(True, chains=True)`): the three `_rows` kernels against
float64 torch autograd and against their plain twins bit for bit, at the smallest shapes that can still go wrong and with NaN wherever
a dead row or window must not be read (1e-5 relative RMS, test_gpu_hifigan_training.py's kernel bound); then the whole node against the
genuine reference's per-stream fixture (tests/golden/make_golden_hifigan_chain_grad.py; outputs 1e-4, gradients 1e-3, the uniform
node test's bounds), its forward's bit-equality with the inference chains path, the padding, reproducibility and row order, the
opt-in, the FULL geometry against the float64 restatement, and Hifi_GAN.train_stage_chains.

The fixture's window counts are 6 / 4 / 6 and then 2 / 6 / 4 (a call's count is always even), so at max_segments = 2 every pass is
full for the streams it runs; the node tests therefore also run at max_segments = 3, where the 4-window stream has ONE live window and
two dead ones in call 0's second pass."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.call_plan import chain_passes
from speech_enhancement_mi_amd.hifigan import Generator, Hifi_GAN
from speech_enhancement_mi_amd.train_net import _p

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402
import make_golden_hifigan_chain_grad as mgc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNUSED = ("deconvlist.3.residual.", "deconvlist.3.residualmask.")


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


def ints(values, dtype):
    return torch.tensor(values, dtype=dtype, device=DEV)


def err(got, want):
    return rel_rms(got.detach().cpu().double().numpy(), want.detach().cpu().double().numpy())


def grads_of(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[n], b[n]) for n in a)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
LIVE = [3, 2, 3, 1, 0, 3, 2, 3, 0, 0, 0]


def lstm_reference(gi, whh, h0, c0, steps, T):
    """float64: the masked recurrence - row b runs steps[b] steps, (h, c) detached at every window seam, zeros after its last step"""
    B, TT, H = gi.shape[0], gi.shape[1], h0.shape[1]
    h, c, outs = h0, c0, []
    for t in range(TT):
        if t % T == 0:
            h, c = h.detach(), c.detach()
        g = gi[:, t] + h @ whh.t()
        c2 = torch.sigmoid(g[:, H:2 * H]) * c + torch.sigmoid(g[:, :H]) * torch.tanh(g[:, 2 * H:3 * H])
        h2 = torch.sigmoid(g[:, 3 * H:]) * torch.tanh(c2)
        on = (t < steps)[:, None]
        outs.append(torch.where(on, h2, torch.zeros_like(h2)))
        h, c = torch.where(on, h2, h), torch.where(on, c2, c)
    return torch.stack(outs, dim=1), h, c


@pytest.mark.parametrize("H", [24, 512])
def test_lstm_rows_training_kernels(H):
    """11 utterances x 3 windows of 5 steps, unsorted live counts: utterance 4 is dead inside the forward's first tile of 8 rows,
    rows 8-10 are a forward tile with nothing to run, the backward's rows 24-32 (utterances 8-10) are fully dead tiles; (h0, c0)
    non-zero.  H = 512 checks the forward only (the backward's tiling does not depend on H)."""
    lib = K._lib()
    B, Nc, T = len(LIVE), 3, 5
    TT = Nc * T
    steps = torch.tensor(LIVE) * T
    gi = rng(1, B, TT, 4 * H).requires_grad_(True)
    whh = rng(2, 4 * H, H, scale=0.3 * (24.0 / H) ** 0.5).requires_grad_(True)
    h0, c0, R = rng(3, B, H, scale=0.5), rng(4, B, H, scale=0.5), rng(5, B, TT, H)
    want_out, want_h, want_c = lstm_reference(gi, whh, h0, c0, steps, T)
    on = (torch.arange(TT)[None, :] < steps[:, None])                     # [B, TT]: the live steps

    gid, whd, h0d, c0d, stepd = dev(gi), dev(whh), dev(h0), dev(c0), ints(steps.tolist(), torch.int32)
    plain = [new(B * TT, H), new(B, H), new(B, H)]
    K._chk(lib.se_hifi_lstm_rows(_p(gid), _p(h0d), _p(c0d), _p(whd), *[_p(t) for t in plain], _p(stepd), B, TT, H, K._st()))
    train = [new(B * TT, H), new(B, H), new(B, H)]
    gates, cs = new(B * TT, 4 * H), new(B * TT, H)
    K._chk(lib.se_hifi_lstm_train_fwd_rows(_p(gid), _p(h0d), _p(c0d), _p(whd), *[_p(t) for t in train], _p(gates), _p(cs), _p(stepd), B, TT, H, K._st()))
    for a, b in zip(plain, train):
        assert torch.equal(a, b)
    assert torch.equal(train[1][4], h0d[4]) and torch.equal(train[2][4], c0d[4])       # steps = 0: the entry state handed on
    assert err(train[0].view(B, TT, H), want_out) <= 1e-5 and err(train[1], want_h) <= 1e-5 and err(train[2], want_c) <= 1e-5
    off = ~on.to(DEV)
    assert torch.isfinite(gates).all() and torch.isfinite(cs).all()
    assert not gates.view(B, TT, 4 * H)[off].any() and not cs.view(B, TT, H)[off].any() and not train[0].view(B, TT, H)[off].any()
    assert gates.view(B, TT, 4 * H)[on.to(DEV)].abs().min() > 0
    if H != 24:
        return
    want_dgi, want_dw = torch.autograd.grad((want_out * R).sum(), [gi, whh])
    Rd, wt = dev(R), whd.t().contiguous()
    hp, cp = new(B * TT, H), new(B * TT, H)
    K._chk(lib.se_train_gru_hprev(_p(train[0]), _p(h0d), _p(hp), B, TT, H, TT, 0, TT, K._st()))
    K._chk(lib.se_train_gru_hprev(_p(cs), _p(c0d), _p(cp), B, TT, H, TT, 0, TT, K._st()))
    assert torch.isfinite(hp).all() and torch.isfinite(cp).all()
    # per utterance, its live windows alone on the plain kernel (before the poison: the slices are copies)
    alone = {}
    for b, n in enumerate(LIVE):
        if n:
            part = [t.view(B, TT, -1)[b, :n * T].contiguous() for t in (Rd, gates, cs, cp)]
            dg1, dc1 = new(n * T, 4 * H), new(n, H)
            K._chk(lib.se_hifi_lstm_bwd(*[_p(t) for t in part], _p(wt), _p(dg1), _p(dc1), 1, n, T, H, K._st()))
            alone[b] = dg1
    # what a dead row would read is NaN
    for t in (Rd, gates, cs, cp):
        t.view(B, TT, -1)[off] = float("nan")
    dg, dc, live = new(B * TT, 4 * H), new(B * Nc, H), ints(LIVE, torch.int32)
    K._chk(lib.se_hifi_lstm_bwd_rows(_p(Rd), _p(gates), _p(cs), _p(cp), _p(wt), _p(dg), _p(dc), _p(live), B, Nc, T, H, K._st()))
    dgv = dg.view(B, TT, 4 * H)
    assert torch.isfinite(dg).all() and not dgv[off].any()
    for b, dg1 in alone.items():
        assert torch.equal(dgv[b, :LIVE[b] * T], dg1), b
    e_gi, e_w = err(dgv, want_dgi), err(K.gemm_tn(dg, hp), want_dw)
    print(f"lstm rows backward: dgi {e_gi:.2e}, dW_hh {e_w:.2e}")
    assert e_gi <= 1e-5 and e_w <= 1e-5
    assert lib.se_hifi_lstm_bwd_rows(_p(Rd), _p(gates), _p(cs), _p(cp), _p(wt), _p(dg), _p(dc), None, B, Nc, T, H, K._st()) != 0   # a null table: an argument error


def test_seqnorm_rows_backward_kernel():
    """three streams at their own steps 0 / 40 / 70 with 3 / 1 / 0 live windows of 3; dy and o are NaN at the dead windows"""
    lib = K._lib()
    B, Nc, C_, T, F = 3, 3, 2, 3, 5
    D, S = C_ * F, Nc * B
    step, cnt = [0, 40, 70], [3, 1, 0]
    o = rng(6, B, Nc, T, D).requires_grad_(True)
    w, bias = (1.0 + rng(7, D, scale=0.3)).requires_grad_(True), rng(8, D, scale=0.3).requires_grad_(True)
    mean_in = rng(9, B, scale=0.2)
    dy = rng(10, S, C_, T, F)
    want = []
    for b in range(B):   # every stream alone
        th = torch.tanh(o)
        gm, st, loss = mean_in[b], float(step[b]), 0.0
        for n in range(cnt[b]):
            alpha = st / (st + D)
            cur = alpha * gm + (1.0 - alpha) * th[b, n].mean()
            y = ((th[b, n] - cur) * w + bias).reshape(T, C_, F).transpose(0, 1)
            loss = loss + (y * dy[n * B + b]).sum()
            gm, st = cur.detach(), st + D
        want.append(torch.autograd.grad(loss, [o, w, bias]) if cnt[b] else None)

    od, wd, bd, md, dyd = dev(o), dev(w), dev(bias), dev(mean_in), dev(dy)
    stepd, cntd = ints(step, torch.int64), ints(cnt, torch.int64)
    wm, mean_out, yk = new(B * Nc), new(B), new(S, C_, T, F)
    K._chk(lib.se_hifi_seqnorm_rows(_p(od), _p(wd), _p(bd), _p(md), _p(stepd), _p(cntd), _p(wm), _p(mean_out), _p(yk), Nc, B, C_, T, F, K._st()))
    dead = torch.tensor([[n >= cnt[b] for n in range(Nc)] for b in range(B)], device=DEV)   # [B, Nc]
    od.view(B, Nc, T, D)[dead] = float("nan")
    dyd.view(Nc, B, C_, T, F)[dead.t()] = float("nan")
    em, do, pw, pb = new(S), new(B * Nc * T, D), new(S, D), new(S, D)
    K._chk(lib.se_hifi_seqnorm_bwd_rows(_p(dyd), _p(od), _p(wd), _p(wm), _p(stepd), _p(cntd), _p(em), _p(do), _p(pw), _p(pb), Nc, B, C_, T, F, K._st()))
    dov, pwv, pbv = do.view(B, Nc, T, D), pw.view(Nc, B, D), pb.view(Nc, B, D)
    assert torch.isfinite(do).all() and torch.isfinite(pw).all() and torch.isfinite(pb).all()
    assert not dov[dead].any() and not pwv[dead.t()].any() and not pbv[dead.t()].any()
    worst = 0.0
    for b in range(B):
        if cnt[b]:
            es = [err(dov[b, :cnt[b]], want[b][0][b, :cnt[b]]), err(pwv[:, b].sum(0), want[b][1]), err(pbv[:, b].sum(0), want[b][2])]
            worst = max(worst, *es)
    print(f"seqnorm rows backward: worst of do / dw / db per stream {worst:.2e}")
    assert worst <= 1e-5
    # every window live at one common step: the plain kernel bit for bit
    od, dyd = dev(o), dev(dy)
    wm2, yk2 = new(B * Nc), new(S, C_, T, F)
    K._chk(lib.se_hifi_seqnorm(_p(od), _p(wd), _p(bd), _p(md), 40.0, _p(wm2), _p(mean_out), _p(yk2), Nc, B, C_, T, F, K._st()))
    plain, rows = [new(S), new(B * Nc * T, D), new(S, D), new(S, D)], [new(S), new(B * Nc * T, D), new(S, D), new(S, D)]
    K._chk(lib.se_hifi_seqnorm_bwd(_p(dyd), _p(od), _p(wd), _p(wm2), 40.0, *[_p(t) for t in plain], Nc, B, C_, T, F, K._st()))
    s40, c3 = ints([40] * B, torch.int64), ints([Nc] * B, torch.int64)
    K._chk(lib.se_hifi_seqnorm_bwd_rows(_p(dyd), _p(od), _p(wd), _p(wm2), _p(s40), _p(c3), *[_p(t) for t in rows], Nc, B, C_, T, F, K._st()))
    assert all(torch.equal(a, b) for a, b in zip(plain, rows))


# ---- the whole node ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gc():
    return np.load(os.path.join(ROOT, "tests", "golden", "hifigan_chain_grad_golden.npz"))


def chains_model(cfg=mh.TINY, max_segments=2):
    m = make_model(cfg).use_hip_training(True, chains=True)
    m.max_segments = max_segments
    return m


def fixture_call(m, gc, c, grad=True, perm=None, pad=None):
    """call c of the fixture on m (rows permuted by perm; pad = (mixture, cotangent) values beyond every length) -> (pred, before)"""
    x, resets, lengths = mgc.batch(c)
    x, R, Rb = torch.from_numpy(x), torch.from_numpy(mgc.padded(gc, c, "R")), torch.from_numpy(mgc.padded(gc, c, "Rb"))
    if pad is not None:
        for b, L in enumerate(lengths):
            x[b, :, L:], R[b, L:], Rb[b, L:] = pad[0], pad[1], pad[1]
    if perm is not None:
        x, R, Rb, resets, lengths = x[perm], R[perm], Rb[perm], [resets[b] for b in perm], [lengths[b] for b in perm]
    m.zero_grad(set_to_none=True)
    with torch.set_grad_enabled(grad):
        pred, before = m.realtime_process_chains(x.to(DEV), resets, lengths)
    if grad:
        assert m._last_path == "kernel" and pred.grad_fn is before.grad_fn and "HifiFunction" in type(pred.grad_fn).__name__
        torch.autograd.backward([pred, before], [R.to(DEV), Rb.to(DEV)])
    return pred.detach(), before.detach()


@pytest.mark.parametrize("max_segments", [2, 3])
def test_chains_node_matches_the_reference_fixture(gc, max_segments):
    """TINY, three streams, both fixture calls in order on one model: call 1 finds per-stream norm step counts, and stream 1 resets
    while it keeps its count.  The measured worst values are in DESIGN.md (HiFi-GAN chunk-chain training)."""
    m = chains_model(max_segments=max_segments)
    for c, (resets, lengths, _) in enumerate(mgc.CALLS):
        pred, before = fixture_call(m, gc, c)
        if c == 0:
            counts = sorted((nb for nb in m._plan([not r for r in resets], lengths, 3, max(lengths), 3).Nb), reverse=True)
            assert counts == [6, 6, 4] and m._last_passes == chain_passes(counts, max_segments)
            assert m._last_passes == ([(0, 2, 3), (2, 2, 3), (4, 2, 2)] if max_segments == 2 else [(0, 3, 3), (3, 3, 3)])
            assert isinstance(m._nstate["step"], list) and len(set(m._nstate["step"])) == 2
        e_out = max(err(v[b:b + 1, :L], torch.from_numpy(gc[f"c{c}_s{b}_{k}"])) for k, v in (("pred", pred), ("before", before))
                    for b, L in enumerate(lengths))
        assert not pred[1, lengths[1]:].any() and not before[1, lengths[1]:].any()
        worst, who = 0.0, None
        for n, p in m.named_parameters():
            ref = gc[f"c{c}_g_{n}"]
            if not np.any(ref):
                assert p.grad is None and n.startswith(UNUSED), n
                continue
            e = rel_rms(mgc.stored(c, n, p.grad.cpu().numpy()), ref)
            worst, who = (e, n) if e > worst else (worst, who)
        print(f"max_segments {max_segments}, call {c}: outputs {e_out:.2e}, worst gradient {worst:.2e} ({who})")
        assert e_out <= 1e-4 and worst <= 1e-3, (c, who)


def test_chains_training_forward_is_the_inference_path_bit_for_bit(gc):
    def session(train):
        m = chains_model(max_segments=3)
        outs = []
        for c in (0, 1, 0):   # the third call, inference, continues either session: call 0's batch again, every stream reset
            pred, before = fixture_call(m, gc, c, grad=train and len(outs) < 2)
            state = [t.clone() for k in ("buf", "h", "c") for t in m._kstate[k]] + [m._nstate["mean"].clone()]
            outs.append((pred, before, state, m._nstate["step"], m._last_passes))
        return outs

    for (p0, b0, s0, n0, l0), (p1, b1, s1, n1, l1) in zip(session(False), session(True)):
        assert torch.equal(p0, p1) and torch.equal(b0, b1) and n0 == n1 and isinstance(n0, list) and l0 == l1
        assert len(s0) == len(s1) and all(torch.equal(x, y) for x, y in zip(s0, s1))


def test_chains_training_never_reads_the_padding(gc):
    runs = []
    for pad in (None, (1e3, float("nan"))):
        m = chains_model(max_segments=3)
        fixture_call(m, gc, 0, grad=False, pad=pad)
        fixture_call(m, gc, 1, pad=pad)
        runs.append(grads_of(m))
    assert all(torch.isfinite(g).all() for g in runs[1].values()) and same(runs[0], runs[1])


def test_chains_training_is_reproducible_and_blind_to_row_order():
    """one call, every stream reset, 8 / 6 / 4 windows (distinct counts: the scheduler's order is the same whatever the caller's), at
    max_segments = 3: passes (0, 3, 3), (3, 3, 3), (6, 2, 1), the 4-window stream with one live window in the second"""
    lengths = [1600, 6400, 3200]
    x = torch.from_numpy(mgc.streams()[..., :6400].copy())
    R, Rb = rng(31, 3, 6400).float(), rng(32, 3, 6400).float()

    def run(perm):
        m = chains_model(max_segments=3)
        pred, before = m.realtime_process_chains(x[perm].to(DEV), [True] * 3, [lengths[b] for b in perm])
        torch.autograd.backward([pred, before], [R[perm].to(DEV), Rb[perm].to(DEV)])
        assert m._last_passes == chain_passes([8, 6, 4], 3) == [(0, 3, 3), (3, 3, 3), (6, 2, 1)]
        return grads_of(m)

    first = run([0, 1, 2])
    assert same(first, run([0, 1, 2])) and same(first, run([2, 0, 1]))


def test_chains_training_is_opt_in(gc):
    x, resets, lengths = mgc.batch(0)
    x = torch.from_numpy(x).to(DEV)
    m = make_model(mh.TINY).use_hip_training(True)
    with pytest.raises(ValueError, match=r"use_hip_training\(False\)"):
        m.realtime_process_chains(x, resets, lengths)
    ref = make_model(mh.TINY, torch.float64).use_hip_kernels(False)
    with torch.no_grad():
        m.realtime_process_chains(x, resets, lengths)
        ref.realtime_process_chains(x.double(), resets, lengths)
    assert isinstance(m._nstate["step"], list) and ref._nstate["step"] == m._nstate["step"]
    u = x[..., :3200].contiguous()
    with pytest.raises(ValueError, match=r"use_hip_training\(False\)"):
        m.realtime_process(u, reset=False)
    # opted in: the uniform call on per-stream step counts is the node
    m.use_hip_training(True, chains=True)
    R, Rb = rng(41, 3, 3200).float().to(DEV), rng(42, 3, 3200).float().to(DEV)
    pred, before = m.realtime_process(u, reset=False)
    assert m._last_path == "kernel" and "HifiFunction" in type(pred.grad_fn).__name__
    torch.autograd.backward([pred, before], [R, Rb])
    p64, b64 = ref.realtime_process(u.double(), reset=False)
    torch.autograd.backward([p64, b64], [R.double(), Rb.double()])
    assert ref._last_path == "torch" and ref._nstate["step"] == m._nstate["step"]
    worst = compare_models(m, ref)
    print(f"uniform call on per-stream step counts: outputs {max(err(pred, p64), err(before, b64)):.2e}, worst gradient {worst:.2e}")
    assert err(pred, p64) <= 1e-4 and err(before, b64) <= 1e-4 and worst <= 1e-3


def compare_models(m, ref):
    worst = 0.0
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        unused = n.startswith(UNUSED)
        assert (p.grad is None) == unused and (q.grad is None) == unused, n
        if not unused:
            worst = max(worst, err(p.grad, q.grad))
    return worst


def test_chains_full_geometry_against_the_float64_restatement():
    lengths = [4800, 1600]
    x = torch.from_numpy(mh.mixture()).to(DEV)[..., :4800].contiguous()
    R, Rb = (rng(s, 2, 4800).float().to(DEV) for s in (21, 22))
    m = chains_model(mh.FULL, max_segments=8)
    pred, before = m.realtime_process_chains(x, [True, True], lengths)
    torch.autograd.backward([pred, before], [R, Rb])
    ref = make_model(mh.FULL, torch.float64)
    p64, b64 = ref.realtime_process_chains(x.double(), [True, True], lengths)
    torch.autograd.backward([p64, b64], [R.double(), Rb.double()])
    assert ref._last_path == "torch" and m._last_path == "kernel" and m._last_passes == [(0, 6, 2)]
    worst = compare_models(m, ref)
    print(f"full geometry chains: outputs {max(err(pred, p64), err(before, b64)):.2e}, worst gradient rel rms {worst:.2e}")
    assert err(pred, p64) <= 1e-4 and err(before, b64) <= 1e-4 and worst <= 1e-3


def test_train_stage_chains_on_the_kernels():
    x, resets, lengths = mgc.batch(0)
    y = np.zeros((3, max(lengths)), np.float32)
    y[:, 3:] = 0.5 * x[:, 0, :-3]
    x, y = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)

    def wrapper():
        w = Hifi_GAN([], [], **mh.TINY).eval()
        w.generator.load_state_dict(mh.state_dict(mh.TINY), strict=True)
        return w.to(DEV)

    ref = wrapper()
    ref.generator.use_hip_kernels(False)
    with torch.no_grad():   # the value only: no graph
        want = float(ref.train_stage_chains(x, y, resets, lengths, stage=2))
    assert ref.generator._last_path == "torch"
    w = wrapper()
    w.generator.use_hip_training(True, chains=True)
    opt = torch.optim.Adam(w.parameters(), lr=1e-4)
    loss = w.train_stage_chains(x, y, resets, lengths, stage=2)
    assert w.generator._last_path == "kernel" and abs(float(loss.detach()) - want) <= 1e-4 * abs(want)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in w.named_parameters() if ".3.residual" not in n)
    opt.step()
    w.generator.reset_norm()
    after = float(w.train_stage_chains(x, y, resets, lengths, stage=2).detach())
    print(f"train_stage_chains: loss {float(loss.detach()):.6f} (restatement {want:.6f}), after one Adam step {after:.6f}")
    assert after < float(loss.detach())
