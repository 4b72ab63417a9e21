"""FullSubNet training over batched chunk chains on the MI355X: TrainableFullSubNet(...).use_hip_kernels(True) with per-utterance flags
and lengths (fsn_train_ws_bytes_chains / fsn_train_fwd_chains / fsn_train_bwd_chains: packed workspace for a fresh, sorted batch; dense
layout with save / zero / restore for a carried one) against the reference fixture, against every utterance alone, against the float64
restatement at the real width, and against the inference engine's own continuation."""
import numpy as np
import pytest
import torch

from conftest import FSN_FULL, FSN_TINY, fsn_spec, rel_rms
from speech_enhancement_mi_amd import synth
from test_fsn_chain_training_cpu import CALLS, FIXTURE, fixture_R, fixture_batch, fixture_gradsum

pytestmark = pytest.mark.gpu

TOL = 1e-4          # outputs against the reference: the project's parity bar
TOL_GRAD = 1e-3     # gradients against the reference: the bar of test_gpu_fsn_training.py against fsn_grad_golden.npz
BAR_ALONE = 2e-6    # batch against each stream alone: BAR_ALONE of the chains tests
STATE_NAMES = ("fh", "fc", "sh", "sc", "mean_fb", "mean_sb", "step_fb", "step_sb")
SE_ERR_ARG, SE_ERR_STATE = -1, -4
K = FSN_TINY["segment_length"]


def _sd(cfg, seed):
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(fsn_spec(cfg), seed=seed).items()}


def _model(cfg, sd, hip, dtype=torch.float32):
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    m = TrainableFullSubNet(**cfg)
    m.load_state_dict(sd)
    return m.cuda().to(dtype).use_hip_kernels(hip)


def _states(m, cfg, B):
    """every exported state name, rows in the caller's order: name -> [B][...]"""
    NL, out = cfg["num_layers"], {}
    for n in STATE_NAMES:
        a = m._eng.export_state(n)
        out[n] = a.reshape(NL, B, -1).transpose(1, 0, 2).reshape(B, -1).copy() if n in ("fh", "fc", "sh", "sc") else a.reshape(B, 1).copy()
    return out


def _rel(a, b):
    return float((a - b).norm() / b.norm())


# ---- 1 / 4. the reference fixture, twice ---------------------------------------------------------------------------------------------
def _fixture_sequence():
    """both CALLS at batch 3 on the kernels -> per call (pred, {name: grad}, states), plus the workspace sizes seen"""
    from speech_enhancement_mi_amd.engine import chain_geometry
    g = np.load(FIXTURE)
    m = _model(FSN_TINY, _sd(FSN_TINY, 0), True)
    out, sizes = [], []
    for c, (flags, lens) in enumerate(CALLS):
        m.zero_grad(set_to_none=True)
        x = fixture_batch(c).cuda()
        eng = m._engine_for(x)
        Nb = chain_geometry(lens, flags, K)["Nb"]
        sizes.append((eng.train_ws_bytes_chains(3, x.shape[2], list(lens), list(flags)), Nb, eng))
        pred = m.realtime_process(x, flag=list(flags), train=False, lengths=list(lens))
        (pred * fixture_R(g, c).cuda()).sum().backward()
        out.append((pred.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, _states(m, FSN_TINY, 3)))
    return out, sizes


@pytest.fixture(scope="module")
def fixture_runs():
    return _fixture_sequence(), _fixture_sequence()


def test_chains_match_the_reference_fixture(fixture_runs):
    g = np.load(FIXTURE)
    (out, sizes), _ = fixture_runs
    for c, (flags, lens) in enumerate(CALLS):
        pred, grads, _ = out[c]
        for b, L in enumerate(lens):
            e = rel_rms(pred[b, :L].cpu().numpy(), g[f"call{c + 1}_utt{b}_pred"])
            print(f"call {c + 1} utterance {b}: pred rel rms {e:.2e}")
            assert e <= TOL, (c, b, e)
            assert bool((pred[b, L:] == 0).all()), (c, b)
        for k, gr in grads.items():
            e = rel_rms(gr.cpu().numpy(), fixture_gradsum(g, c, k))
            print(f"call {c + 1} {k}: {e:.2e}")
            assert e <= TOL_GRAD, f"call {c + 1} {k}: rel rms {e:.2e}"
    # call 1 is fresh with non-increasing window counts: the packed layout, S[0] = sum_n bact(n) = sum_b Nb[b] rows.  A layout of S[0]
    # rows is what the plain call gives one stream with S[0] windows; the chains header (8 B floats of plan + S[0] row-table ints,
    # rounded up to 64 floats) comes on top.
    (ws1, Nb1, eng), (ws2, Nb2, _) = sizes
    hdr = lambda floats: 4 * ((floats + 63) // 64 * 64)
    assert Nb1 == sorted(Nb1, reverse=True) and len(set(Nb1)) > 1
    assert ws1 == eng.train_ws_bytes(1, sum(Nb1)) + hdr(8 * 3 + sum(Nb1))
    assert ws1 < eng.train_ws_bytes(3, max(Nb1))
    # call 2 is carried, one reset among continuing streams, unsorted counts: the dense layout
    assert Nb2 != sorted(Nb2, reverse=True) and CALLS[1][0] == (True, False, True)
    assert ws2 == eng.train_ws_bytes(3, max(Nb2)) + hdr(8 * 3)


def test_two_runs_are_bit_identical(fixture_runs):
    (a, _), (b, _) = fixture_runs
    for (pa, ga, sa), (pb, gb, sb) in zip(a, b):
        assert torch.equal(pa, pb)
        assert all(torch.equal(ga[k], gb[k]) for k in ga)
        assert all(np.array_equal(sa[n], sb[n]) for n in STATE_NAMES)


# ---- 2. each utterance against itself alone --------------------------------------------------------------------------------------------
def test_each_utterance_equals_its_own_chain_alone():
    """Three calls; in engine order: fresh and permuted (packed), carried with a reset and unsorted counts (dense), carried with
    non-increasing counts (packed while carried).  One utterance ends two windows before the longest in every call."""
    from speech_enhancement_mi_amd.engine import chain_geometry
    calls = (((False, False, False), (3400, 8000, 5200)), ((True, False, True), (4800, 1500, 7000)), ((True, True, True), (4800, 6400, 1700)))
    for flags, lens in calls:
        Nb = chain_geometry(lens, flags, K)["Nb"]
        assert max(Nb) - min(Nb) >= 2, Nb
    mix = synth.synth_utterances(3, 21000, 3, seed=33)[0]
    sd = _sd(FSN_TINY, 0)
    m, m1 = _model(FSN_TINY, sd, True), _model(FSN_TINY, sd, True)
    lo = [0, 0, 0]
    chunks = []
    for flags, lens in calls:
        chunks.append([mix[b:b + 1, :, lo[b]:lo[b] + lens[b]].copy() for b in range(3)])
        lo = [lo[b] + lens[b] for b in range(3)]
    alone = {}
    for b in range(3):
        for c, (flags, lens) in enumerate(calls):
            p = m1.realtime_process(torch.from_numpy(chunks[c][b]).cuda(), flag=flags[b], train=False)
            assert p.requires_grad
            alone[c, b] = (p.detach().cpu().numpy()[0], _states(m1, FSN_TINY, 1))
    worst = 0.0
    for c, (flags, lens) in enumerate(calls):
        x = np.full((3, 3, max(lens)), 3.0, np.float32)
        for b in range(3):
            x[b, :, :lens[b]] = chunks[c][b][0]
        pred = m.realtime_process(torch.from_numpy(x).cuda(), flag=list(flags), train=False, lengths=list(lens))
        assert pred.requires_grad
        pred, st = pred.detach().cpu().numpy(), _states(m, FSN_TINY, 3)
        for b in range(3):
            ref_p, ref_s = alone[c, b]
            e = rel_rms(pred[b, :lens[b]], ref_p)
            worst = max(worst, e)
            assert e <= BAR_ALONE, (c, b, e)
            assert np.all(pred[b, lens[b]:] == 0.0), (c, b)
            for n in STATE_NAMES:
                got, ref = st[n][b], ref_s[n][0]
                if n.startswith("step"):
                    assert np.array_equal(got, ref), (c, b, n, got, ref)
                elif not np.any(ref):
                    assert np.max(np.abs(got)) <= 1e-6, (c, b, n)
                else:
                    e = rel_rms(got, ref)
                    worst = max(worst, e)
                    assert e <= BAR_ALONE, (c, b, n, e)
    print(f"batch against each utterance alone: largest error {worst:.3e}")


# ---- 3. gradients at the real width against float64 -----------------------------------------------------------------------------------
def test_full_config_chains_vs_float64_restatement():
    """FSN_FULL, utterances of 1.0 s and 0.6 s (fresh: packed), then flags [True, False] (carried, unsorted: dense); loss sum(pred * R).
    Per tensor the kernels must be as close to the float64 restatement as max(2 x the fp32 restatement's own error, 5e-5)."""
    sd = _sd(FSN_FULL, 3)
    calls = (((False, False), (16000, 9600)), ((True, False), (8000, 12800)))
    mix = synth.synth_utterances(2, 16000 + 12800, 3, seed=91)[0]
    xs, Rs, lo = [], [], [0, 0]
    for c, (flags, lens) in enumerate(calls):
        x = np.full((2, 3, max(lens)), 3.0, np.float32)
        for b in range(2):
            x[b, :, :lens[b]] = mix[b, :, lo[b]:lo[b] + lens[b]]
        lo = [lo[b] + lens[b] for b in range(2)]
        xs.append(torch.from_numpy(x).cuda())
        Rs.append(torch.from_numpy(np.random.default_rng(50 + c).standard_normal((2, max(lens))).astype(np.float32)).cuda())

    def run(hip, dtype):
        m = _model(FSN_FULL, sd, hip, dtype)
        out = []
        for c, (flags, lens) in enumerate(calls):
            m.zero_grad(set_to_none=True)
            pred = m.realtime_process(xs[c].to(dtype), flag=list(flags), train=False, lengths=list(lens))
            (pred * Rs[c].to(dtype)).sum().backward()
            out.append({k: p.grad.detach().double().clone() for k, p in m.named_parameters()})
        return out

    g64, gt, gh = run(False, torch.float64), run(False, torch.float32), run(True, torch.float32)
    flat = lambda g: torch.cat([v.flatten() for v in g.values()])
    bad = []
    for c in range(2):
        e_t, e_h = _rel(flat(gt[c]), flat(g64[c])), _rel(flat(gh[c]), flat(g64[c]))
        print(f"call {c + 1}: flat-gradient error vs float64: torch fp32 {e_t:.2e}, HIP kernels {e_h:.2e}")
        for k in g64[c]:
            assert float(g64[c][k].norm()) > 0, k
            et, eh = _rel(gt[c][k], g64[c][k]), _rel(gh[c][k], g64[c][k])
            print(f"call {c + 1} {k}: |g| {float(g64[c][k].norm()):.2e}  torch fp32 {et:.2e}  HIP {eh:.2e}")
            if not eh <= max(2.0 * et, 5e-5):
                bad.append((c, k, eh, et))
    assert not bad, bad


# ---- 5. a uniform batch is the scalar call ------------------------------------------------------------------------------------------
def test_uniform_list_is_the_scalar_call():
    mix, _ = synth.synth_utterances(2, 8000, 3, seed=7)
    sd = _sd(FSN_TINY, 0)
    outs = []
    for listed in (False, True):
        m = _model(FSN_TINY, sd, True)
        got = []
        for a, b, flag in ((0, 4800, False), (4800, 8000, True)):
            x = torch.from_numpy(mix[..., a:b].copy()).cuda()
            kw = dict(flag=[flag, flag], lengths=[b - a, b - a]) if listed else dict(flag=flag)
            m.zero_grad(set_to_none=True)
            pred = m.realtime_process(x, train=False, **kw)
            pred.square().sum().backward()
            got += [pred.detach()] + [p.grad.clone() for p in m.parameters()] + [torch.from_numpy(v) for v in _states(m, FSN_TINY, 2).values()]
        outs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 6. training and inference share the state --------------------------------------------------------------------------------------
def test_ragged_training_call_continues_as_inference_chains():
    """After a ragged training call, a flagged chains chunk under no_grad (FsnEngine.realtime_process_chains on the same engine) is what
    the inference engine gives after ITS OWN ragged first call: the training forward leaves the inference engine's state, bit for bit."""
    from speech_enhancement_mi_amd.fullsubnet import FullSubNet
    sd = _sd(FSN_TINY, 0)
    m = _model(FSN_TINY, sd, True)
    ref = FullSubNet(**FSN_TINY)
    ref.load_state_dict(sd)
    ref = ref.cuda()
    (f1, l1), (f2, l2) = CALLS
    x1, x2 = fixture_batch(0).cuda(), fixture_batch(1).cuda()
    p_train = m.realtime_process(x1, flag=list(f1), train=False, lengths=list(l1))
    assert p_train.requires_grad
    with torch.no_grad():
        p_inf = ref.realtime_process(x1, flag=list(f1), train=False, lengths=list(l1))
        assert rel_rms(p_train.detach().cpu().numpy(), p_inf.cpu().numpy()) <= 1e-6
        c_train = m.realtime_process(x2, flag=list(f2), train=False, lengths=list(l2))
        c_inf = ref.realtime_process(x2, flag=list(f2), train=False, lengths=list(l2))
    assert not c_train.requires_grad and torch.equal(c_train, c_inf)


# ---- 7. the full loss on a ragged batch ---------------------------------------------------------------------------------------------
def test_full_loss_on_a_ragged_batch():
    sd = _sd(FSN_TINY, 0)
    flags, lens = CALLS[0]
    mix, clean = synth.synth_utterances(3, max(lens), 3, seed=41)
    for b, L in enumerate(lens):
        mix[b, :, L:] = 3.0
    x = torch.from_numpy(mix).cuda()
    src = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    length = torch.tensor(lens, dtype=torch.int64, device="cuda")
    vals = []
    for hip in (False, True):
        m = _model(FSN_TINY, sd, hip)
        pred, crm, s, xf = m.realtime_process(x, src, list(flags), train=False, lengths=length)
        loss = m.compute_loss(src[:, 0], pred, xf, s, crm, length)[0]
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        vals.append(float(loss.detach()))
    l_t, l_h = vals
    print(f"ragged batch full loss: torch fp32 {l_t:.7f}  HIP {l_h:.7f}  relative difference {abs(l_h - l_t) / abs(l_t):.2e}")
    assert np.isfinite(l_h)
    assert abs(l_h - l_t) <= 1e-5 * abs(l_t)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------
def test_planner_errors_leave_the_carried_state_intact():
    g = np.load(FIXTURE)
    m = _model(FSN_TINY, _sd(FSN_TINY, 0), True)
    x1 = fixture_batch(0).cuda()
    eng = m._engine_for(x1)
    lens = list(CALLS[0][1])
    L = x1.shape[2]
    spec = torch.zeros(8, 3 * 3, eng.T, eng.F, 2, device="cuda")
    ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")

    def refused(code, text, B, ln, fl):
        with pytest.raises(RuntimeError, match=f"error {code}:.*{text}"):
            eng.train_ws_bytes_chains(B, L, ln, fl)
        with pytest.raises(RuntimeError, match=f"error {code}:.*{text}"):
            eng.train_fwd_chains(spec[:, :B * 3].contiguous(), B, L, ln, fl, ws, 8)

    refused(SE_ERR_STATE, "carries no state", 3, lens, [True, False, False])       # nothing is carried yet
    m.realtime_process(x1, flag=[False] * 3, train=False, lengths=lens)
    before = _states(m, FSN_TINY, 3)
    refused(SE_ERR_STATE, "carried state holds 3 streams", 2, lens[:2], [True, False])
    refused(SE_ERR_ARG, "outside", 3, [lens[0], 0, lens[2]], [True, False, True])
    refused(SE_ERR_ARG, "outside", 3, [lens[0], L + 1, lens[2]], [True, False, True])
    after = _states(m, FSN_TINY, 3)
    assert all(np.array_equal(before[n], after[n]) for n in STATE_NAMES)
    flags2, lens2 = CALLS[1]
    pred = m.realtime_process(fixture_batch(1).cuda(), flag=list(flags2), train=False, lengths=list(lens2))
    for b, l in enumerate(lens2):
        assert rel_rms(pred[b, :l].detach().cpu().numpy(), g[f"call2_utt{b}_pred"]) <= TOL, b
