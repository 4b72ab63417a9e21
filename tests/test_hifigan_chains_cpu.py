"""CPU tests of the HiFi-GAN generator's chunk chains (hifigan.Generator.realtime_process_chains) on the torch restatement: a batch of
streams equals every stream alone, bit for bit - both outputs, every carried row, the running mean and the norm's step count, which
is per stream once the streams advance by different window counts; the chains form stays pinned to the genuine reference's fixture
while a neighbour resets and has another length; the uniform triage; `_nstate["step"]` as an int and as a list; reset_norm(streams);
the refusals; the Hifi_GAN wrapper.  Window counts at segment_length 3200: a reset of 1600 / 4800 / 6400 / 9600 samples has
4 / 6 / 8 / 10 windows, a continuation of <= 1599 / 3200 / 4800 / 8000 samples 2 / 4 / 6 / 8."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd.hifigan import Generator, Hifi_GAN

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402

# three consecutive calls over four streams: (resets, lengths); stream 3 is the long one, stream 1 starts a new utterance in call 2
CALLS = [([True, True, True, True], [4800, 1600, 6400, 9600]),
         ([False, True, False, False], [1000, 4800, 3200, 1599]),
         ([False, False, False, False], [3200, 3200, 1599, 8000])]
WINDOWS = [[6, 4, 8, 10], [2, 6, 4, 2], [4, 4, 2, 8]]
B = 4
D = 13 * 8   # the tiny geometry's bottleneck features: the norm's step count advances by D per window


def make_model(tag="tiny", **change):
    cfg = dict(dict(mh.GEOMS)[tag], **change)
    m = Generator(**cfg).eval()
    m.load_state_dict(mh.state_dict(cfg), strict=True)
    return m


def scenario(calls, seed, nstreams):
    """-> per call (clean batch [B, 3, Lmax], the same with 1e3 beyond every length, resets, lengths)"""
    out = []
    for c, (resets, lens) in enumerate(calls):
        resets, lens = resets[:nstreams], lens[:nstreams]
        mix = torch.from_numpy(synth.synth_utterances(nstreams, max(lens), 3, seed=seed + c)[0])
        dirty = mix.clone()
        for b, L in enumerate(lens):
            dirty[b, :, L:] = 1e3
        out.append((mix, dirty, resets, lens))
    return out


def same_row(batch_state, b, alone_state):
    """row b of the batch's `_tstate` is the B = 1 model's"""
    return (all(torch.equal(t[b:b + 1], a) for t, a in zip(batch_state["buf"], alone_state["buf"]))
            and all(torch.equal(h[b:b + 1], ha) and torch.equal(c[b:b + 1], ca) for (h, c), (ha, ca) in zip(batch_state["hc"], alone_state["hc"])))


@pytest.fixture(scope="module")
def chains():
    """The scenario once, in passes of 3 windows: the batch model after every call against four models that each serve one stream.
    -> (batch model, alone models, the scenario): every comparison of the three calls is made here, on the way."""
    batch, alone = make_model(), [make_model() for _ in range(B)]
    for m in [batch] + alone:
        m.max_segments = 3
    scen = scenario(CALLS, 140, B)
    steps = []
    with torch.no_grad():
        for c, (mix, dirty, resets, lens) in enumerate(scen):
            pred, before = batch.realtime_process_chains(dirty, torch.tensor(resets), lens)
            assert batch._last_path == "torch" and pred.shape == before.shape == (B, max(lens))
            assert torch.isfinite(pred).all() and torch.isfinite(before).all()
            for b, (r, L) in enumerate(zip(resets, lens)):
                want = alone[b].realtime_process(mix[b:b + 1, :, :L], reset=r)
                for got, w in zip((pred, before), want):
                    assert torch.equal(got[b, :L], w[0]), (c, b)
                    assert torch.count_nonzero(got[b, L:]) == 0, (c, b)
                assert same_row(batch._tstate, b, alone[b]._tstate), (c, b)
                assert torch.equal(batch._nstate["mean"][b:b + 1], alone[b]._nstate["mean"]), (c, b)
                assert Generator._steps_of(batch._nstate, B)[b] == alone[b]._nstate["step"], (c, b)
            steps.append(batch._nstate["step"])
    return batch, alone, steps


def test_chains_equal_every_stream_alone(chains):
    """the fixture compares outputs, carried rows, means and counts call by call; here: the count never restarts, whatever resets[b] says"""
    steps = chains[2]
    assert steps == [[sum(w[b] for w in WINDOWS[:c + 1]) * D for b in range(B)] for c in range(3)]


def test_norm_step_is_an_int_while_the_streams_agree_and_a_list_after(chains):
    """after the ragged scenario the counts differ: a list.  A uniform call on that state goes on per stream, against the models that
    serve one stream each; uniform calls on a uniform state keep an int."""
    batch, alone, steps = chains
    assert all(isinstance(s, list) and len(s) == B and all(isinstance(v, int) for v in s) for s in steps)
    mix = torch.from_numpy(synth.synth_utterances(B, 3200, 3, seed=150)[0])
    kept = batch._nstate["step"]
    assert isinstance(kept, list)
    with torch.no_grad():
        pred, before = batch.realtime_process(mix, reset=False)
        for b in range(B):
            want = alone[b].realtime_process(mix[b:b + 1], reset=False)
            assert torch.equal(pred[b:b + 1], want[0]) and torch.equal(before[b:b + 1], want[1]), b
            assert same_row(batch._tstate, b, alone[b]._tstate)
            assert torch.equal(batch._nstate["mean"][b:b + 1], alone[b]._nstate["mean"])
    assert batch._nstate["step"] == [s + 4 * D for s in kept] == [a._nstate["step"] for a in alone]
    m = make_model()
    with torch.no_grad():
        m.realtime_process(mix[:2], reset=True)
        assert m._nstate["step"] == 6 * D and isinstance(m._nstate["step"], int)
        m.realtime_process_chains(mix[:2], [False, False], [3200, 3200])
        assert m._nstate["step"] == 10 * D and isinstance(m._nstate["step"], int)
        m.realtime_process_chains(mix[:2], [True, False], [1600, 3200])      # 4 and 4 windows: chains, and the counts still agree
        assert m._nstate["step"] == 14 * D and isinstance(m._nstate["step"], int)
        m.realtime_process_chains(mix[:2], [False, False], [1000, 3200])     # 2 and 4
        assert m._nstate["step"] == [16 * D, 18 * D]
        with pytest.raises(ValueError, match="one norm step count"):         # forward() has one count for the batch
            m(torch.from_numpy(mh.spectrum()).expand(2, -1, -1, -1, -1))


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_chains_match_reference_fixture(tag):
    """Streams 0 and 1: the fixture's two utterances through its three calls (reset, continue, reset again); stream 2: other data,
    other lengths, and a continuation where the fixture resets.  A neighbour's reset or length must not reach the norm that survives
    resets: the fixture's outputs, its mean and its step hold on streams 0 and 1."""
    hg = np.load(os.path.join(ROOT, "tests", "golden", "hifigan_golden.npz"))
    m = make_model(tag)
    mix = mh.mixture()
    other = synth.synth_utterances(1, 9600, 3, seed=23)[0]
    extra = [(1600, True), (6400, False), (3200, False)]
    with torch.no_grad():
        for c, ((a, b, reset), (L2, r2)) in enumerate(zip(mh.CALLS, extra)):
            x = np.full((3, 3, max(b - a, L2)), 1e3, np.float32)
            x[:2, :, :b - a] = mix[..., a:b]
            x[2, :, :L2] = other[0, :, c * 1600:c * 1600 + L2]
            outs = m.realtime_process_chains(torch.from_numpy(x), [reset, reset, r2], [b - a, b - a, L2])
            assert m._last_path == "torch"
            for name, v in zip(("pred", "before"), outs):
                v = v.numpy()
                e = rel_rms(v[:2, :b - a], hg[f"{tag}_c{c}_{name}"])
                print(f"HiFi-GAN chains restatement vs reference fixture: {tag} call {c} {name} rel rms {e:.3e}")
                assert np.isfinite(v).all() and e <= 1e-5, (tag, c, name, e)
                assert np.count_nonzero(v[:2, b - a:]) == 0 and np.count_nonzero(v[2, L2:]) == 0
            assert Generator._steps_of(m._nstate, 3)[:2] == [int(hg[f"{tag}_c{c}_step"][0])] * 2
            assert np.abs(m._nstate["mean"].numpy()[:2] - hg[f"{tag}_c{c}_mean"]).max() <= 1e-6


def test_a_uniform_batch_is_realtime_process():
    a, b = make_model(), make_model()
    mix = torch.from_numpy(mh.mixture())
    with torch.no_grad():
        for lo, hi, reset in mh.CALLS:
            x = mix[..., lo:hi]
            want = a.realtime_process(x, reset=reset)
            got = b.realtime_process_chains(x, torch.tensor([reset, reset]), [hi - lo, hi - lo])
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert b._nstate["step"] == a._nstate["step"] and isinstance(b._nstate["step"], int)
            assert torch.equal(b._nstate["mean"], a._nstate["mean"])
            assert all(same_row(b._tstate, r, Generator._state_row(a._tstate, r, 2)) for r in range(2))
        got = b.realtime_process_chains(mix[..., :3200], True)               # one value for the batch
        want = a.realtime_process(mix[..., :3200], reset=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_reset_norm_of_one_stream_hands_the_slot_to_a_new_caller():
    m, others, fresh = make_model(), make_model(), make_model()
    scen = scenario(CALLS[:2], 160, 3)
    new = torch.from_numpy(synth.synth_utterances(3, 4800, 3, seed=170)[0])
    m.reset_norm(streams=[1])                                                # nothing carried: nothing to do
    assert m._nstate is None
    with torch.no_grad():
        for _, dirty, resets, lens in scen:
            m.realtime_process_chains(dirty, resets, lens)
            others.realtime_process_chains(dirty, resets, lens)
        before = m._nstate
        m.reset_norm(streams=[1])
        assert m._nstate is not before and float(m._nstate["mean"][1]) == 0.0 and Generator._steps_of(m._nstate, 3)[1] == 0
        assert torch.equal(m._nstate["mean"][[0, 2]], before["mean"][[0, 2]]) and torch.equal(before["mean"], others._nstate["mean"])
        got = m.realtime_process_chains(new, [False, True, False], [3200, 4800, 1000])
        want = others.realtime_process_chains(new, [False, True, False], [3200, 4800, 1000])
        alone = fresh.realtime_process(new[1:2], reset=True)
    for g, w, a in zip(got, want, alone):
        assert torch.equal(g[1:2], a) and not torch.equal(w[1:2], a)         # stream 1: a fresh model's result
        assert torch.equal(g[[0, 2]], w[[0, 2]])                             # the others: as if nothing had happened
    assert torch.equal(m._nstate["mean"][1:2], fresh._nstate["mean"]) and Generator._steps_of(m._nstate, 3)[1] == fresh._nstate["step"]
    with pytest.raises(ValueError, match="streams 0 .. 2"):
        m.reset_norm(streams=[3])
    m.reset_norm()
    assert m._nstate is None


def test_refusals_name_the_cause_and_leave_the_state():
    m = make_model()
    mix = torch.from_numpy(synth.synth_utterances(3, 3200, 3, seed=7)[0])
    with torch.no_grad():
        with pytest.raises(ValueError, match="there is none"):              # a stream continues, nothing carried
            m.realtime_process_chains(mix, [False, True, False])
        assert m._tstate is None and m._nstate is None
        m.realtime_process_chains(mix[:2], [True, True], [3200, 1000])
        kept, norm = m._tstate, m._nstate
        with pytest.raises(ValueError, match="batch of 2 utterances, got 3"):   # the norm's running mean is of another batch size
            m.realtime_process_chains(mix, [False, True, False])
        with pytest.raises(ValueError, match="flags for a batch of 2"):
            m.realtime_process_chains(mix[:2], [True, False, True])
        with pytest.raises(ValueError, match="lengths must be 2 values"):
            m.realtime_process_chains(mix[:2], [True, False], [3200, 3201])
        with pytest.raises(TypeError, match="reference cannot either"):
            m.realtime_process_chains(mix[:2], [True, False], post=False)
        with pytest.raises(ValueError, match="one `reset`"):
            m.realtime_process(mix[:2], reset=[True, False])
        assert m._tstate is kept and m._nstate is norm
        m.reset_norm()
        with pytest.raises(ValueError, match="one of 2"):                   # and with the norm forgotten, so are the buffers and (h, c)
            m.realtime_process_chains(mix, [False, True, False])
        assert m._tstate is kept and m._nstate is None
        m._nstate = norm
        m._last_path = "kernel"                                            # the carried state belongs to the other path
        with pytest.raises(RuntimeError, match="other path"):
            m.realtime_process_chains(mix[:2], [True, False])
        assert m._tstate is kept and m._nstate is norm


def test_hifi_gan_wrapper_returns_the_generators_pred():
    cfg = dict(mh.TINY)
    net = Hifi_GAN([512, 1024], [40, 80], **cfg).eval()
    net.load_state_dict({"generator." + k: v for k, v in mh.state_dict(cfg).items()}, strict=True)
    g = make_model()
    _, dirty, resets, lens = scenario(CALLS[:1], 180, 2)[0]
    with torch.no_grad():
        y = net.realtime_process_chains(dirty, resets, lens)
        want = g.realtime_process_chains(dirty, resets, lens)[0]
    assert y.shape == (2, 4800) and torch.equal(y, want)
