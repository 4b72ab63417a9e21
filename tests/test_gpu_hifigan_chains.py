"""GPU tests of the HiFi-GAN generator's chunk chains on the kernel path (hifigan.Generator._kernel_process, se_hifi_lstm_rows,
se_hifi_seqnorm_rows): the two per-stream kernels bit-equal to the plain ones on every row alone, a batch of chains bit-equal to every
stream alone through the uniform kernel path (both outputs, every carried row, the running mean and the norm's step count, whatever
the pass split), the pass schedule, the genuine reference's fixture, the restatement's chains form, the refusals, and the uniform call
as the chains runner's identity case.  Window counts at segment_length 3200: a reset of 1600 / 4800 / 6400 / 9600 samples has
4 / 6 / 8 / 10 windows, a continuation of <= 1599 / 3200 / 4800 / 8000 samples 2 / 4 / 6 / 8."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.call_plan import chain_geometry
from speech_enhancement_mi_amd.gtsa import chain_passes
from speech_enhancement_mi_amd.hifigan import Generator
from speech_enhancement_mi_amd.train_net import _p
from test_gpu_hifigan import DEV, dev, make_model, mh, rng

pytestmark = pytest.mark.gpu

# three consecutive calls over four streams: (resets, lengths); stream 3 is the long one, so the others end while passes still run
CALLS = [([True, True, True, True], [4800, 1600, 6400, 9600]),
         ([False, True, False, False], [1000, 4800, 3200, 1599]),
         ([False, False, False, False], [3200, 3200, 1599, 8000])]


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
@pytest.mark.parametrize("H", [16, 512])
def test_lstm_rows_kernel(H):
    """steps unsorted, a finished row inside a live tile of 8, and a second tile (rows 8, 9) with nothing to run"""
    In, TT, B, steps = 24, 5, 10, [2, 5, 0, 3, 5, 1, 4, 3, 0, 0]
    torch.manual_seed(H)
    ref = torch.nn.LSTM(In, H, 1, batch_first=True).double()
    x, h0, c0 = rng(1, B, TT, In), rng(2, B, H, scale=0.5), rng(3, B, H, scale=0.5)
    gi = K._gemm(dev(x.reshape(B * TT, In)), dev(ref.weight_ih_l0), dev(ref.bias_ih_l0 + ref.bias_hh_l0)).view(B, TT, 4 * H)
    h0d, c0d, whh = dev(h0), dev(c0), dev(ref.weight_hh_l0)
    keep = (h0d.clone(), c0d.clone())
    lib = K._lib()

    def rows(counts):
        out, hk, ck = nan(B, TT, H), nan(B, H), nan(B, H)
        s_d = torch.tensor(counts, dtype=torch.int32, device=DEV)
        K._chk(lib.se_hifi_lstm_rows(_p(gi), _p(h0d), _p(c0d), _p(whh), _p(out), _p(hk), _p(ck), _p(s_d), B, TT, H, K._st()))
        return out, hk, ck

    def plain(gi_, h_, c_, n, tt):
        out, hk, ck = nan(n, tt, H), nan(n, H), nan(n, H)
        K._chk(lib.se_hifi_lstm(_p(gi_), _p(h_), _p(c_), _p(whh), _p(out), _p(hk), _p(ck), n, tt, H, K._st()))
        return out, hk, ck

    out, hk, ck = rows(steps)
    assert torch.isfinite(out).all() and torch.isfinite(hk).all() and torch.isfinite(ck).all()
    for b, s in enumerate(steps):
        if s:
            o1, h1, c1 = plain(gi[b, :s].contiguous(), h0d[b:b + 1].contiguous(), c0d[b:b + 1].contiguous(), 1, s)
            assert torch.equal(out[b, :s], o1[0]) and torch.equal(hk[b], h1[0]) and torch.equal(ck[b], c1[0]), b
        else:
            assert torch.equal(hk[b], h0d[b]) and torch.equal(ck[b], c0d[b]), b
        assert torch.count_nonzero(out[b, s:]) == 0, b
    assert torch.equal(h0d, keep[0]) and torch.equal(c0d, keep[1])           # the state it started from is left alone
    for a, w in zip(rows([TT] * B), plain(gi, h0d, c0d, B, TT)):
        assert torch.equal(a, w)
    # the live part against float64 nn.LSTM, the bar of test_lstm_kernel
    got, want = [], []
    for s in sorted(set(steps) - {0}):
        o64, (h64, c64) = ref(x[:, :s], (h0[None], c0[None]))
        for b in [b for b, sb in enumerate(steps) if sb == s]:
            got += [out[b, :s].reshape(-1), hk[b], ck[b]]
            want += [o64[b].reshape(-1), h64[0, b], c64[0, b]]
    e = rel_rms(torch.cat(got).cpu().double().numpy(), torch.cat(want).numpy())
    print(f"lstm rows H={H}: rel rms of the live part {e:.2e}")
    assert e <= 1e-5


@torch.no_grad()
def test_seqnorm_rows_kernel():
    B, Nc, T, C_, F, cnt = 3, 3, 3, 8, 13, [3, 1, 0]
    D = C_ * F
    step = [0, 5 * D, 2 * D]
    od, wd, bd, md = dev(rng(6, B, Nc, T, D, scale=1.5)), dev(1.0 + 0.25 * rng(7, D)), dev(0.25 * rng(8, D)), dev(rng(9, B, scale=0.1))
    lib = K._lib()

    def rows(steps_, counts):
        y, wm, mo = nan(Nc * B, C_, T, F), nan(B * Nc), nan(B)
        s_d, c_d = (torch.tensor(v, dtype=torch.int64, device=DEV) for v in (steps_, counts))
        K._chk(lib.se_hifi_seqnorm_rows(_p(od), _p(wd), _p(bd), _p(md), _p(s_d), _p(c_d), _p(wm), _p(mo), _p(y), Nc, B, C_, T, F, K._st()))
        return y.view(Nc, B, C_, T, F), wm.view(B, Nc), mo

    def plain(o_, m_, step_, n, nc):
        y, wm, mo = nan(nc * n, C_, T, F), nan(n * nc), nan(n)
        K._chk(lib.se_hifi_seqnorm(_p(o_), _p(wd), _p(bd), _p(m_), float(step_), _p(wm), _p(mo), _p(y), nc, n, C_, T, F, K._st()))
        return y.view(nc, n, C_, T, F), wm.view(n, nc), mo

    y, wm, mo = rows(step, cnt)
    assert torch.isfinite(y).all() and torch.isfinite(wm).all() and torch.isfinite(mo).all()   # the dead windows too
    for b, c in enumerate(cnt):
        if c:
            y1, wm1, mo1 = plain(od[b, :c].contiguous(), md[b:b + 1].contiguous(), step[b], 1, c)
            assert torch.equal(y[:c, b], y1[:, 0]) and torch.equal(wm[b, :c], wm1[0]) and torch.equal(mo[b], mo1[0]), b
        else:
            assert torch.equal(mo[b], md[b]), b
    assert not torch.equal(mo[1], md[1])
    for a, w in zip(rows([5 * D] * B, [Nc] * B), plain(od, md, 5 * D, B, Nc)):
        assert torch.equal(a, w)


# ---- a batch of chains against every stream alone ------------------------------------------------------------------------------------
def scenario(calls, nstreams, seed):
    """-> per call (clean batch [B, 3, Lmax], the same with 1e3 beyond every length, resets, lengths), on the GPU"""
    out = []
    for c, (resets, lens) in enumerate(calls):
        resets, lens = resets[:nstreams], lens[:nstreams]
        mix = torch.from_numpy(synth.synth_utterances(nstreams, max(lens), 3, seed=seed + c)[0])
        dirty = mix.clone()
        for b, L in enumerate(lens):
            dirty[b, :, L:] = 1e3
        out.append((mix.to(DEV), dirty.to(DEV), resets, lens))
    return out


def run_chains(tag, scen, max_segments):
    """-> (both outputs per call, the model): the scenario as chains calls, the schedule checked on the way"""
    m = make_model(tag)
    m.max_segments = max_segments
    ys = []
    for _, dirty, resets, lens in scen:
        ys.append(m.realtime_process_chains(dirty, torch.tensor(resets), torch.tensor(lens)))
        assert m._last_path == "kernel"
        Nb = sorted(chain_geometry(lens, [not r for r in resets], 3200)["Nb"], reverse=True)
        assert m._last_passes == chain_passes(Nb, max_segments) and sum(p[1] for p in m._last_passes) == Nb[0]
    return ys, m


def check_against_alone(tag, scen, ys, m, max_segments):
    B = len(scen[0][2])
    alone = [make_model(tag) for _ in range(B)]
    for c, (mix, _, resets, lens) in enumerate(scen):
        for b, (r, L) in enumerate(zip(resets, lens)):
            alone[b].max_segments = max_segments
            want = alone[b].realtime_process(mix[b:b + 1, :, :L].contiguous(), reset=r)
            for got, w in zip(ys[c], want):
                assert torch.isfinite(got).all() and torch.equal(got[b, :L], w[0]), (tag, c, b)
                assert torch.count_nonzero(got[b, L:]) == 0, (tag, c, b)
    steps = Generator._steps_of(m._nstate, B)
    for b in range(B):   # and what the last call leaves is every stream's own: buffers, (h, c), the running mean, the step count
        sa, sb = alone[b]._kstate, m._kstate
        for key in ("buf", "h", "c"):
            for i, t in enumerate(sb[key]):
                assert torch.isfinite(t).all() and torch.equal(t[b], sa[key][i][0]), (b, key, i)
        assert torch.equal(m._nstate["mean"][b], alone[b]._nstate["mean"][0]) and steps[b] == alone[b]._nstate["step"], b


def same(ya, yb):
    return all(torch.equal(a[i], b[i]) for a, b in zip(ya, yb) for i in range(2))


@torch.no_grad()
def test_chains_equal_every_stream_alone_tiny():
    scen = scenario(CALLS, 4, 80)
    ys, m = run_chains("tiny", scen, 3)
    assert m._last_passes == [(0, 3, 4), (3, 3, 3), (6, 2, 1)]            # call 3: window counts 4 4 2 8
    assert isinstance(m._nstate["step"], list)
    check_against_alone("tiny", scen, ys, m, 3)
    ys_whole, mw = run_chains("tiny", scen, 1000)                         # one pass per call
    ys_again, ma = run_chains("tiny", scen, 3)
    assert same(ys, ys_whole) and same(ys, ys_again)
    for other in (mw, ma):
        assert torch.equal(other._nstate["mean"], m._nstate["mean"]) and other._nstate["step"] == m._nstate["step"]
        assert all(torch.equal(a, b) for key in ("buf", "h", "c") for a, b in zip(other._kstate[key], m._kstate[key]))


@torch.no_grad()
def test_chains_equal_every_stream_alone_full():
    scen = scenario(CALLS[:2], 3, 90)
    ys, m = run_chains("full", scen, 3)
    check_against_alone("full", scen, ys, m, 3)


# ---- the genuine reference and the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "full"])
@torch.no_grad()
def test_kernel_chains_match_reference_fixture(tag):
    """Streams 0 and 1: the fixture's two utterances through its three calls (reset, continue, reset again); stream 2: other data,
    other lengths, and a continuation where the fixture resets."""
    hg = np.load(os.path.join(ROOT, "tests", "golden", "hifigan_golden.npz"))
    m = make_model(tag)
    mix = mh.mixture()
    other = synth.synth_utterances(1, 9600, 3, seed=23)[0]
    extra = [(1600, True), (6400, False), (3200, False)]
    for c, ((a, b, reset), (L2, r2)) in enumerate(zip(mh.CALLS, extra)):
        x = np.full((3, 3, max(b - a, L2)), 1e3, np.float32)
        x[:2, :, :b - a] = mix[..., a:b]
        x[2, :, :L2] = other[0, :, c * 1600:c * 1600 + L2]
        outs = m.realtime_process_chains(torch.from_numpy(x).to(DEV), [reset, reset, r2], [b - a, b - a, L2])
        assert m._last_path == "kernel"
        for name, v in zip(("pred", "before"), outs):
            v = v.cpu().numpy()
            e = rel_rms(v[:2, :b - a], hg[f"{tag}_c{c}_{name}"])
            print(f"HiFi-GAN kernel chains vs reference fixture: {tag} call {c} {name} rel rms {e:.3e}")
            assert np.isfinite(v).all() and e <= 1e-4, (tag, c, name, e)
            assert np.count_nonzero(v[:2, b - a:]) == 0 and np.count_nonzero(v[2, L2:]) == 0
        assert Generator._steps_of(m._nstate, 3)[:2] == [int(hg[f"{tag}_c{c}_step"][0])] * 2
        assert float(np.abs(m._nstate["mean"].cpu().numpy()[:2] - hg[f"{tag}_c{c}_mean"]).max()) <= 1e-5


@pytest.mark.parametrize("tag", ["tiny", "full"])
@torch.no_grad()
def test_kernel_chains_match_restatement_chains(tag):
    mk, mt = make_model(tag), make_model(tag).use_hip_kernels(False)
    for c, (_, dirty, resets, lens) in enumerate(scenario(CALLS[:2], 3, 100)):
        yk = mk.realtime_process_chains(dirty, resets, lens)
        yt = mt.realtime_process_chains(dirty, resets, lens)
        assert mk._last_path == "kernel" and mt._last_path == "torch"
        for name, k, t in zip(("pred", "before"), yk, yt):
            err = rel_rms(k.cpu().numpy(), t.cpu().numpy())
            print(f"HiFi-GAN kernel chains vs restatement chains: {tag} call {c} {name} rel rms {err:.3e}")
            assert torch.isfinite(k).all() and err <= 1e-4, (tag, c, name, err)
        assert mk._nstate["step"] == mt._nstate["step"]
        assert float((mk._nstate["mean"].cpu() - mt._nstate["mean"].cpu()).abs().max()) <= 1e-5


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_refusals_leave_the_carried_state():
    (_, x0, r0, l0), (_, x1, r1, l1) = scenario(CALLS[:2], 3, 110)
    m, clean = make_model("tiny"), make_model("tiny")
    with pytest.raises(ValueError, match="there is none"):              # a stream continues, nothing carried
        m.realtime_process_chains(x1, r1, l1)
    assert m._kstate is None and m._nstate is None
    m.realtime_process_chains(x0[:2], r0[:2], l0[:2])
    kept, norm = m._kstate, m._nstate
    with pytest.raises(ValueError, match="batch of 2 utterances, got 3"):   # the norm's running mean is of another batch size
        m.realtime_process_chains(x1, r1, l1)
    with pytest.raises(TypeError, match="reference cannot either"):
        m.realtime_process_chains(x1[:2], r1[:2], l1[:2], post=False)
    assert m._kstate is kept and m._nstate is norm
    m.reset_norm()
    with pytest.raises(ValueError, match="one of 2"):                   # and with the norm forgotten, so are the buffers and (h, c)
        m.realtime_process_chains(x1, r1, l1)
    assert m._kstate is kept
    m._nstate = norm
    y = m.realtime_process_chains(x1[:2], r1[:2], l1[:2])               # the refused calls touched nothing
    clean.realtime_process_chains(x0[:2], r0[:2], l0[:2])
    assert same([y], [clean.realtime_process_chains(x1[:2], r1[:2], l1[:2])])
    x2 = x1[:2, :, :3200].contiguous()
    assert same([m.realtime_process(x2, reset=False)], [clean.realtime_process(x2, reset=False)])   # and a uniform continuation


# ---- the uniform call -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_uniform_call_is_the_chains_runner_with_every_stream_in_every_pass():
    """B = 2: a reset of 4800 samples (6 windows), then a continuation of 3200 (4 windows), in passes of 3: realtime_process, the same
    through realtime_process_chains (bit-equal, the scalar kernels), and forced onto the chains form - stream 1 one sample short, which
    leaves its window count as it is - on stream 0's samples."""
    mix = torch.from_numpy(synth.synth_utterances(2, 8000, 3, seed=130)[0]).to(DEV)
    uni, same_call, chains = make_model("tiny"), make_model("tiny"), make_model("tiny")
    uni.max_segments = same_call.max_segments = chains.max_segments = 3
    for (a, b), r, passes in (((0, 4800), True, [(0, 3, 2), (3, 3, 2)]), ((4800, 8000), False, [(0, 3, 2), (3, 1, 2)])):
        x = mix[..., a:b].contiguous()
        yu = uni.realtime_process(x, reset=r)
        assert uni._last_path == "kernel" and uni._last_passes == passes
        ys = same_call.realtime_process_chains(x, [r, r], [b - a, b - a])
        assert same([yu], [ys]) and torch.equal(same_call._nstate["mean"], uni._nstate["mean"])
        assert same_call._nstate["step"] == uni._nstate["step"] and isinstance(uni._nstate["step"], int)
        yc = chains.realtime_process_chains(x, [r, r], [b - a, b - a - 1])
        assert chains._last_passes == passes and chains._nstate["step"] == uni._nstate["step"]
        assert all(torch.isfinite(v).all() for v in yu) and torch.equal(yu[0][0], yc[0][0]) and torch.equal(yu[1][0], yc[1][0]), r
        assert torch.equal(chains._nstate["mean"][0], uni._nstate["mean"][0])


@torch.no_grad()
def test_a_uniform_call_honours_a_carried_list_of_step_counts():
    """after a ragged call the counts differ; the uniform continuation that follows runs the scalar LSTM and the per-stream scan"""
    (mix, dirty, r0, l0), = scenario(CALLS[:1], 3, 135)
    m, alone = make_model("tiny"), [make_model("tiny") for _ in range(3)]
    m.realtime_process_chains(dirty, r0, l0)
    assert isinstance(m._nstate["step"], list)
    x = torch.from_numpy(synth.synth_utterances(3, 3200, 3, seed=136)[0]).to(DEV)
    y = m.realtime_process(x, reset=False)
    for b in range(3):
        alone[b].realtime_process(mix[b:b + 1, :, :l0[b]].contiguous(), reset=True)
        want = alone[b].realtime_process(x[b:b + 1].contiguous(), reset=False)
        assert torch.equal(y[0][b], want[0][0]) and torch.equal(y[1][b], want[1][0]), b
        assert torch.equal(m._nstate["mean"][b], alone[b]._nstate["mean"][0]) and m._nstate["step"][b] == alone[b]._nstate["step"]
