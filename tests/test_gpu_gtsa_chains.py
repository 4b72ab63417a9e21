"""GPU tests of GTSA chunk chains on the kernel path (gtsa.GTSA._kernel_process, se_gtsa_tape_rows, se_gtsa_lastframes_rows): the two
per-stream copy kernels exactly against indexing, a batch of chains bit-equal to every stream alone through the uniform kernel path
(outputs and carried state, whatever the pass split), the pass schedule, the genuine reference's fixture, the restatement's chains
form, the refusals, and the uniform call as the chains runner's identity case.  Window counts at segment_length 3200: a reset of 1600 / 4800 / 6400 / 9600 samples has 4 / 6 / 8 / 10 windows,
a continuation of <= 1599 / 3200 / 4800 / 8000 samples 2 / 4 / 6 / 8."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd import train_ops as K
from speech_enhancement_mi_amd.call_plan import chain_geometry
from speech_enhancement_mi_amd.gtsa import chain_passes
from speech_enhancement_mi_amd.train_net import _p
from test_gpu_gtsa import DEV, Fs, T, dev, kernel_spectrum, make_model, mgt, rng

pytestmark = pytest.mark.gpu

# three consecutive calls, per stream (flags, lengths); stream 3 is the long one, so the others end while passes still run
CALLS = [([False, False, False, False], [4800, 1600, 6400, 9600]),
         ([True, False, True, True], [1000, 4800, 3200, 1599]),
         ([True, True, True, True], [3200, 3200, 1599, 8000])]


def cnt_of(values):
    return torch.tensor(values, dtype=torch.int64, device=DEV)


# ---- the two kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["even", "odd"])
@torch.no_grad()
def test_tape_rows_kernel(case):
    B, U, Hh, D, ld = dict(even=(3, 2, 3, 67, 208), odd=(3, 7, 1, 5, 16))[case]
    maxlen, Nc, cnt = 50, 4, [4, 1, 0]
    S, HD = Nc * B, Hh * D
    kn, vn = rng(61, Nc, B, U, T, Hh, D).float(), rng(62, Nc, B, U, T, Hh, D).float()
    kc, vc = rng(63, B, U, Hh, maxlen, D).float(), rng(64, B, U, Hh, maxlen, D).float()
    kv = torch.zeros(S, U, T, 2 * ld)                     # k | v rows of stride ld inside one buffer of stride 2 ld
    kv[..., :HD], kv[..., ld:ld + HD] = kn.reshape(S, U, T, HD), vn.reshape(S, U, T, HD)
    kv_d, kc_d, vc_d = dev(kv), dev(kc), dev(vc)
    lib = K._lib()

    def run(fn, *count):
        ko, vo = torch.full_like(kc_d, float("nan")), torch.full_like(vc_d, float("nan"))
        K._chk(fn(_p(kv_d), _p(kv_d, ld), _p(kc_d), _p(vc_d), _p(ko), _p(vo), *count, 2 * ld, Nc, B, U, Hh, D, T, maxlen, K._st()))
        return ko.cpu(), vo.cpu()

    c_d = cnt_of(cnt)
    ko, vo = run(lib.se_gtsa_tape_rows, _p(c_d))
    for got, carried, new in ((ko, kc, kn), (vo, vc, vn)):
        tape = torch.cat([carried, new.permute(1, 2, 4, 0, 3, 5).reshape(B, U, Hh, Nc * T, D)], dim=3)   # [B, U, Hh, maxlen + Nc T, D]
        want = torch.stack([tape[b, :, :, c * T:c * T + maxlen] for b, c in enumerate(cnt)])
        assert torch.equal(got, want)
    assert torch.equal(ko[2], kc[2]) and torch.equal(vo[2], vc[2])       # cnt = 0: the carried part
    full_d = cnt_of([Nc] * B)
    ka, va = run(lib.se_gtsa_tape_rows, _p(full_d))
    kb, vb = run(lib.se_gtsa_tape)
    assert torch.equal(ka, kb) and torch.equal(va, vb)


@torch.no_grad()
def test_lastframes_rows_kernel():
    B, Nc, cnt = 3, 3, [3, 1, 0]
    x, buf = rng(65, Nc * B, 5, T, Fs).float(), rng(66, B, 5, 2, Fs).float()
    x_d, buf_d, c_d = x.to(DEV), buf.to(DEV), cnt_of(cnt)
    out = torch.full((B, 5, 2, Fs), float("nan"), device=DEV)
    K._chk(K._lib().se_gtsa_lastframes_rows(_p(x_d), _p(buf_d), _p(out), _p(c_d), Nc, B, T, Fs, K._st()))
    want = torch.stack([x[(c - 1) * B + b, :, T - 2:] if c else buf[b] for b, c in enumerate(cnt)])
    assert torch.equal(out.cpu(), want)


# ---- a batch of chains against every stream alone ------------------------------------------------------------------------------------
def scenario(calls, B, seed):
    """-> per call (clean batch [B, 3, Lmax] zero beyond every length, the same with garbage there, flags, lengths), on the GPU"""
    out = []
    for c, (flags, lens) in enumerate(calls):
        flags, lens = flags[:B], lens[:B]
        mix = torch.from_numpy(synth.synth_utterances(B, max(lens), 3, seed=seed + c)[0])
        dirty = mix.clone()
        for b, L in enumerate(lens):
            dirty[b, :, L:] = 1e3
        out.append((mix.to(DEV), dirty.to(DEV), flags, lens))
    return out


def run_chains(tag, scen, max_segments):
    """-> (outputs per call, the model): the scenario as chains calls, the schedule checked on the way"""
    m = make_model(tag)
    m.max_segments = max_segments
    ys = []
    for _, dirty, flags, lens in scen:
        ys.append(m.realtime_process(dirty, flag=torch.tensor(flags), lengths=torch.tensor(lens)))
        assert m._last_path == "kernel"
        Nb = sorted(chain_geometry(lens, flags, 3200)["Nb"], reverse=True)
        assert m._last_passes == chain_passes(Nb, max_segments) and sum(p[1] for p in m._last_passes) == Nb[0]
    return ys, m


def check_against_alone(tag, scen, ys, m, max_segments):
    B = len(scen[0][2])
    alone = [make_model(tag) for _ in range(B)]
    for c, (mix, _, flags, lens) in enumerate(scen):
        assert torch.isfinite(ys[c]).all()
        for b, (f, L) in enumerate(zip(flags, lens)):
            alone[b].max_segments = max_segments
            want = alone[b].realtime_process(mix[b:b + 1, :, :L].contiguous(), flag=f)
            assert torch.equal(ys[c][b, :L], want[0]), (tag, c, b)
            assert torch.count_nonzero(ys[c][b, L:]) == 0, (tag, c, b)
    for b in range(B):   # and the state the last call leaves is every stream's own
        sa, sb = alone[b]._kstate, m._kstate
        assert torch.equal(sb["buf"][b], sa["buf"][0]), b
        for key in ("k", "v"):
            for i, t in enumerate(sb[key]):
                assert torch.isfinite(t).all() and torch.equal(t.view(B, -1)[b], sa[key][i].view(-1)), (b, key, i)


@torch.no_grad()
def test_chains_equal_every_stream_alone_tiny():
    scen = scenario(CALLS, 4, 80)
    ys, m = run_chains("tiny", scen, 3)
    assert m._last_passes == [(0, 3, 4), (3, 3, 3), (6, 2, 1)]            # call 3: window counts 4 4 2 8
    check_against_alone("tiny", scen, ys, m, 3)
    ys_whole, _ = run_chains("tiny", scen, 1000)                          # one pass per call
    ys_again, _ = run_chains("tiny", scen, 3)
    for a, b, c in zip(ys, ys_whole, ys_again):
        assert torch.equal(a, b) and torch.equal(a, c)


@torch.no_grad()
def test_chains_equal_every_stream_alone_full():
    scen = scenario(CALLS[:2], 3, 90)
    ys, m = run_chains("full", scen, 3)
    check_against_alone("full", scen, ys, m, 3)


# ---- the genuine reference and the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "full"])
@torch.no_grad()
def test_kernel_chains_match_reference_fixture(tag):
    """Streams 0 and 1: the fixture's two utterances as its two chunks; stream 2: 1600 fresh samples, then a reset with 6400."""
    gg = np.load(os.path.join(ROOT, "tests", "golden", "gtsa_golden.npz"))
    m = make_model(tag)
    mix = mgt.mixture()
    other = synth.synth_utterances(1, 8000, 3, seed=19)[0]
    for c, ((a, b, flag), L2) in enumerate(zip(mgt.CHUNKS, (1600, 6400))):
        x = np.zeros((3, 3, max(b - a, L2)), np.float32)
        x[:2, :, :b - a] = mix[..., a:b]
        x[2, :, :L2] = other[0, :, c * 1600:c * 1600 + L2]
        y = m.realtime_process(torch.from_numpy(x).to(DEV), flag=[flag, flag, False], lengths=[b - a, b - a, L2]).cpu().numpy()
        assert m._last_path == "kernel"
        err = rel_rms(y[:2, :b - a], gg[f"{tag}_out{c}"])
        print(f"GTSA kernel chains vs reference fixture: {tag} chunk {c} rel rms {err:.3e}")
        assert np.isfinite(y).all() and err <= 1e-4, (tag, c, err)
        assert np.count_nonzero(y[:2, b - a:]) == 0 and np.count_nonzero(y[2, L2:]) == 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
@torch.no_grad()
def test_kernel_chains_match_restatement_chains(tag):
    mk, mt = make_model(tag), make_model(tag)
    mt.use_hip_kernels(False)
    mt.spectrum = kernel_spectrum(mt)
    for c, (_, dirty, flags, lens) in enumerate(scenario(CALLS[:2], 3, 100)):
        yk = mk.realtime_process(dirty, flag=flags, lengths=lens)
        yt = mt.realtime_process(dirty, flag=flags, lengths=lens)
        assert mk._last_path == "kernel" and mt._last_path == "torch"
        err = rel_rms(yk.cpu().numpy(), yt.cpu().numpy())
        print(f"GTSA kernel chains vs restatement chains: {tag} call {c} rel rms {err:.3e}")
        assert torch.isfinite(yk).all() and err <= 1e-4, (tag, c, err)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_refusals_leave_the_carried_state():
    scen = scenario(CALLS[:2], 3, 110)
    (_, x0, f0, l0), (_, x1, f1, l1) = scen
    m, clean = make_model("tiny"), make_model("tiny")
    with pytest.raises(ValueError, match="there is none"):              # mixed flags, nothing carried
        m.realtime_process(x1, flag=f1, lengths=l1)
    m.realtime_process(x0[:2], flag=[False, False], lengths=l0[:2])
    with pytest.raises(ValueError, match="one of 2"):                   # mixed flags after a call of another batch size
        m.realtime_process(x1, flag=f1, lengths=l1)
    m.realtime_process(x0, flag=f0, lengths=l0)
    with pytest.raises(ValueError, match="one of 3"):
        m.realtime_process(x1[:2], flag=[True, False], lengths=l1[:2])
    y = m.realtime_process(x1, flag=f1, lengths=l1)                     # the failed call touched nothing
    clean.realtime_process(x0, flag=f0, lengths=l0)
    assert torch.equal(y, clean.realtime_process(x1, flag=f1, lengths=l1))
    with pytest.raises(ValueError, match="one of 3"):
        m.realtime_process(x1[:2], flag=[True, False], lengths=l1[:2])
    x2 = x1[..., :3200].contiguous()
    assert torch.equal(m.realtime_process(x2, flag=True), clean.realtime_process(x2, flag=True))   # and a uniform continuation


@torch.no_grad()
def test_a_refused_chains_call_leaves_the_carried_state():
    """a flag set, a carried batch of 2, a call of 3: refused before the state is touched, and the chain of 2 goes on as if never asked"""
    (_, x0, f0, l0), (_, x1, f1, l1) = scenario(CALLS[:2], 3, 120)
    m, clean = make_model("tiny"), make_model("tiny")
    m.realtime_process(x0[:2], flag=f0[:2], lengths=l0[:2])
    kept = m._kstate
    with pytest.raises(ValueError, match="one of 2"):
        m.realtime_process(x1, flag=f1, lengths=l1)
    assert m._kstate is kept
    y = m.realtime_process(x1[:2], flag=f1[:2], lengths=l1[:2])
    clean.realtime_process(x0[:2], flag=f0[:2], lengths=l0[:2])
    assert torch.equal(y, clean.realtime_process(x1[:2], flag=f1[:2], lengths=l1[:2]))


# ---- the uniform call -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def test_uniform_call_is_the_chains_runner_with_every_stream_in_every_pass():
    """B = 2: a reset of 4800 samples (6 windows), then a continuation of 3200 (4 windows), in passes of 3.  Against the same two calls
    forced onto the chains form - stream 1 one sample short, which leaves its window count as it is - on stream 0's samples."""
    mix = torch.from_numpy(synth.synth_utterances(2, 8000, 3, seed=130)[0]).to(DEV)
    uni, chains = make_model("tiny"), make_model("tiny")
    uni.max_segments = chains.max_segments = 3
    for (a, b), f, passes in (((0, 4800), False, [(0, 3, 2), (3, 3, 2)]), ((4800, 8000), True, [(0, 3, 2), (3, 1, 2)])):
        x = mix[..., a:b].contiguous()
        yu = uni.realtime_process(x, flag=f)
        assert uni._last_path == "kernel" and uni._last_passes == passes
        yc = chains.realtime_process(x, flag=[f, f], lengths=[b - a, b - a - 1])
        assert chains._last_passes == passes
        assert torch.isfinite(yu).all() and torch.equal(yu[0], yc[0]), f
