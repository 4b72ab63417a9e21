"""CPU tests of the drop-in HiFi-GAN generator (speech_enhancement_mi_amd/hifigan.py): checkpoint layout against the genuine reference's,
the weight-norm fold against torch's own, the torch restatement against the reference fixture (tests/golden/make_golden_hifigan.py)
including the running mean that survives reset(), the batched windows against the window loop, chunking, the refusals, and the kernel
path's geometry limits."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_rms
from speech_enhancement_mi_amd import synth
from speech_enhancement_mi_amd.call_plan import call_plan, windows
from speech_enhancement_mi_amd.hifigan import Generator, Hifi_GAN, fold_weight_norm

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_hifigan as mh  # noqa: E402

GEOMS = dict(mh.GEOMS)


@pytest.fixture(scope="module")
def hkeys():
    with open(os.path.join(ROOT, "tests", "golden", "hifigan_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def hg():
    return np.load(os.path.join(ROOT, "tests", "golden", "hifigan_golden.npz"))


def make_model(tag, dtype=torch.float32, **change):
    cfg = dict(GEOMS[tag], **change)
    m = Generator(**cfg).eval().to(dtype)
    m.load_state_dict(mh.state_dict(cfg), strict=True)
    return m


def mix64():
    return torch.from_numpy(mh.mixture()).double()


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_state_dict_layout(tag, hkeys):
    m = Generator(**GEOMS[tag])
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == hkeys[tag] and len(got) == 157
    assert [[k, list(s)] for k, s in mh.spec_of(GEOMS[tag])] == hkeys[tag]
    assert sum(p.numel() for p in m.parameters()) == hkeys[tag + "_params"]
    names = [k for k, _ in got]
    assert "convlist.0.net.0.weight_g" in names and "deconvlist.0.residualmask.weight_v" in names and "gru.fc_output_layer.weight_g" in names
    assert not any(k.endswith(".weight") and "norm" not in k for k in names)


def test_full_parameter_count(hkeys):
    assert hkeys["full_params"] == 7923878


def test_synthetic_weights_alias_and_gain():
    sd = synth.hifigan_state_dict(mh.spec_of(mh.TINY), seed=0)
    assert np.array_equal(sd["convlist.1.conv.weight_g"], sd["convlist.1.net.0.weight_g"])
    assert np.array_equal(sd["postnet.3.conv.weight_v"], sd["postnet.3.net.0.weight_v"])
    v = sd["postnet.5.conv.weight_v"].astype(np.float64).reshape(128, -1)
    ratio = sd["postnet.5.conv.weight_g"].reshape(-1) / np.sqrt((v ** 2).sum(1))
    assert 0.9 * synth.HIFIGAN_GAIN / 1.7 <= ratio.min() and ratio.max() <= 1.1 * synth.HIFIGAN_GAIN / 1.7 + 1e-6


@pytest.mark.parametrize("kind", ["conv", "deconv", "fc"])
def test_fold_equals_torch_weight_norm(kind):
    """g * v / ||v|| per dim-0 row in float64 against torch.nn.utils.weight_norm's own weight; dim 0 of a ConvTranspose2d weight is
    the INPUT channel."""
    torch.manual_seed(3)
    mod = dict(conv=torch.nn.Conv2d(5, 7, (5, 3)), deconv=torch.nn.ConvTranspose2d(6, 4, (5, 3)), fc=torch.nn.Linear(16, 24))[kind].double()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = torch.nn.utils.weight_norm(mod)
    with torch.no_grad():
        ref.weight_g.mul_(torch.rand_like(ref.weight_g) + 0.5)
        ref.weight_v.mul_(1.7)
        want = torch._weight_norm(ref.weight_v, ref.weight_g, 0)
    got = fold_weight_norm(ref.weight_g, ref.weight_v)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12
    if kind == "deconv":
        assert ref.weight_g.shape == (6, 1, 1, 1)


# The restatement and the reference run the same float32 torch operators in another order (every window of a pass at once against the
# window loop); each is about 2e-6 from float64 on this input (make_golden_hifigan.py's precheck asserts 5e-6), so 1e-5 - a tenth
# of the project's bar - holds both.
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_restatement_matches_reference(tag, hg):
    m = make_model(tag)
    mix = mh.mixture()
    steps = []
    with torch.no_grad():
        for c, (a, b, reset) in enumerate(mh.CALLS):
            pred, before = m.realtime_process(torch.from_numpy(mix[..., a:b].copy()), reset=reset)
            assert m._last_path == "torch"
            for name, v in (("pred", pred), ("before", before)):
                e = rel_rms(v.numpy(), hg[f"{tag}_c{c}_{name}"])
                assert e <= 1e-5, (tag, c, name, e)
            assert m._nstate["step"] == int(hg[f"{tag}_c{c}_step"][0])
            assert np.abs(m._nstate["mean"].numpy() - hg[f"{tag}_c{c}_mean"]).max() <= 1e-6
            steps.append(m._nstate["step"])
    # the third call resets the model and the count goes on: the running mean survives reset()
    assert steps[2] > steps[1] > steps[0] and steps[2] - steps[1] == steps[0]


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_forward_and_taps_match_reference(tag, hg):
    m = make_model(tag)
    m.taps = {}
    with torch.no_grad():
        y, yb = m(torch.from_numpy(mh.spectrum()))
    assert rel_rms(y.numpy(), hg[f"{tag}_fwd"]) <= 1e-5 and rel_rms(yb.numpy(), hg[f"{tag}_fwd_before"]) <= 1e-5
    for name in mh.TAPS:
        v = m.taps[name].numpy()
        assert list(v.shape) == list(hg[f"{tag}_tap_{name}_shape"]), name
        got = v.reshape(-1)[mh.tap_index(name, v.size)]
        assert rel_rms(got, hg[f"{tag}_tap_{name}"]) <= 1e-5, (name, rel_rms(got, hg[f"{tag}_tap_{name}"]))


def _state_close(a, b, tol):
    for x, y in zip(a["buf"], b["buf"]):
        assert torch.allclose(x, y, rtol=0, atol=tol * float(y.abs().max() + 1))
    for (h1, c1), (h2, c2) in zip(a["hc"], b["hc"]):
        assert torch.allclose(h1, h2, rtol=0, atol=tol) and torch.allclose(c1, c2, rtol=0, atol=tol)


def test_realtime_process_equals_the_window_loop():
    """realtime_process (every window of a pass at once) against a loop of forward() (the reference's form), in float64: the same two
    outputs, the same carried state and the same running mean, over a reset=True and a reset=False call."""
    mt, mw = make_model("tiny", torch.float64), make_model("tiny", torch.float64)
    mix = mix64()
    with torch.no_grad():
        for a, b, reset in mh.CALLS[:2]:
            x = mix[..., a:b]
            plan = call_plan(not reset, None, 2, b - a, 3200, 160, 400)
            X = mt.spectrum(windows(plan, x))
            (Y, Yb), mt._tstate, mt._nstate = mt._pass(X, mt._tstate if not reset else None, mt._nstate)
            if reset:
                mw.reset()
            loop = [mw(X[:, :, n]) for n in range(plan.N)]
            assert rel_rms(Y.numpy(), torch.stack([l[0] for l in loop], dim=1).numpy()) < 1e-12
            assert rel_rms(Yb.numpy(), torch.stack([l[1] for l in loop], dim=1).numpy()) < 1e-12
            _state_close(mt._tstate, mw._tstate, 1e-12)
            assert mt._nstate["step"] == mw._nstate["step"] and torch.allclose(mt._nstate["mean"], mw._nstate["mean"], rtol=0, atol=1e-14)


def test_max_segments_does_not_change_the_result():
    m1, m2 = make_model("tiny", torch.float64), make_model("tiny", torch.float64)
    m1.max_segments, m2.max_segments = 1, 1000
    mix = mix64()
    with torch.no_grad():
        for a, b, reset in mh.CALLS:
            for y1, y2 in zip(m1.realtime_process(mix[..., a:b], reset=reset), m2.realtime_process(mix[..., a:b], reset=reset)):
                assert rel_rms(y1.numpy(), y2.numpy()) < 1e-12
    _state_close(m1._tstate, m2._tstate, 1e-12)
    assert m1._nstate["step"] == m2._nstate["step"]


def test_whole_call_equals_the_chunked_call_where_the_contract_says():
    """Windows are 3200 samples at a step of 1600, and an output sample is the mean of the two windows that cover it.  A chunk of 4800
    samples sees its own samples only, so the windows starting at -3200 .. 1600 are those of the whole call (same content, same order,
    same state before them); the window at 3200 is not (zeros beyond 4800).  Samples [0, 3200) are covered by the former alone: there
    the two calls agree.  Beyond, the chunked call is another computation (the reference's too)."""
    m1, m2 = make_model("tiny", torch.float64), make_model("tiny", torch.float64)
    mix = mix64()
    with torch.no_grad():
        whole = m1.realtime_process(mix, reset=True)
        first = m2.realtime_process(mix[..., :4800], reset=True)
        second = m2.realtime_process(mix[..., 4800:], reset=False)
    for w, f, s in zip(whole, first, second):
        assert w.shape == (2, 8000) and f.shape == (2, 4800) and s.shape == (2, 3200)
        assert rel_rms(f[:, :3200].numpy(), w[:, :3200].numpy()) < 1e-12
        assert rel_rms(f[:, 3200:].numpy(), w[:, 3200:4800].numpy()) > 1e-6


def test_reset_norm_makes_a_fresh_model():
    m = make_model("tiny")
    x = torch.from_numpy(mh.mixture()[..., :4800].copy())
    with torch.no_grad():
        first = m.realtime_process(x, reset=True)
        again = m.realtime_process(x, reset=True)     # the running mean carried on: another result
        m.reset_norm()
        fresh = m.realtime_process(x, reset=True)
    assert torch.equal(first[0], fresh[0]) and torch.equal(first[1], fresh[1])
    assert not torch.equal(first[0], again[0])


def test_norm_state_survives_reset_and_refuses_another_batch():
    m = make_model("tiny")
    mix = torch.from_numpy(mh.mixture())
    with torch.no_grad():
        m.realtime_process(mix[..., :3200], reset=True)
        m.reset()
        assert m._tstate is None and m._nstate is not None and m._nstate["mean"].shape == (2,)
        with pytest.raises(ValueError, match="batch of 2 utterances, got 3"):
            m.realtime_process(mix[[0, 1, 0], :, :3200], reset=True)
        assert m._nstate["mean"].shape == (2,)
        # a carried batch of 1 is what the reference's broadcast accepts
        m.reset_norm()
        m.realtime_process(mix[:1, :, :3200], reset=True)
        y, _ = m.realtime_process(mix[..., :3200], reset=True)
        assert y.shape == (2, 3200) and m._nstate["mean"].shape == (2,)


def test_hifi_gan_wrapper_loads_a_checkpoint_with_discriminators():
    cfg = dict(mh.TINY)
    sd = {"generator." + k: v for k, v in mh.state_dict(cfg).items()}
    sd["discriminator.0.discriminators.0.convs.0.weight_g"] = torch.zeros(3)
    sd["discriminator.1.discriminators.2.conv_post.bias"] = torch.zeros(1)
    net = Hifi_GAN([512, 1024], [40, 80], **cfg).eval()
    net.load_state_dict(sd, strict=True)
    assert not hasattr(net, "remove_weight_norm") and not hasattr(net, "discriminator")
    g = make_model("tiny")
    x = torch.from_numpy(mh.mixture()[..., :4800].copy())
    with torch.no_grad():
        y = net(x)
        want = g.realtime_process(x, reset=False)[0]
    assert torch.equal(y, want)


def test_post_false_and_list_reset_are_refused():
    m = make_model("tiny")
    x = torch.from_numpy(mh.mixture()[..., :3200].copy())
    with torch.no_grad():
        with pytest.raises(TypeError, match="reference cannot either"):
            m.realtime_process(x, post=False)
        with pytest.raises(ValueError, match="one `reset`"):
            m.realtime_process(x, reset=[True, False])
        y, yb = m(torch.from_numpy(mh.spectrum()), post=False)
    assert yb is None and y.shape == (1, 201, 21, 2)
    assert m._tstate is not None


def test_restatement_is_differentiable():
    m = make_model("tiny").train()
    pred, before = m.realtime_process(torch.from_numpy(mh.mixture()[..., :3200].copy()), reset=True)
    (pred.pow(2).mean() + before.pow(2).mean()).backward()
    assert m._last_path == "torch"
    for name, p in m.named_parameters():
        if name.startswith("deconvlist.3.residual"):   # the last block has no skip: the reference builds the pair and never calls it
            assert p.grad is None, name
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(m.postnet[5].conv.weight_g.grad.abs().max()) > 0 and float(m.convlist[0].conv.weight_v.grad.abs().max()) > 0


@pytest.mark.parametrize("change,limit", [(dict(num_inputs=2), "num_inputs = 2"), (dict(kernel_size=5), "kernel_size = 5"), (dict(hidden=20), "hidden = 20"),
                                          (dict(num_channels=[4, 8, 8, 8, 8]), "history (k - 1) * 2^(L - 1) = 32 frames")])
def test_kernel_path_refuses_unsupported_geometry(change, limit):
    err = Generator(**dict(mh.TINY, **change)).kernel_geometry_error()
    assert err is not None and limit in err, err


def test_kernel_path_accepts_both_fixture_geometries():
    for cfg in (mh.TINY, mh.FULL):
        assert Generator(**cfg).kernel_geometry_error() is None
