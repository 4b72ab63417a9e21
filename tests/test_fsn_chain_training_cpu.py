"""FullSubNet training over batched chunk chains, CPU side: the C ABI additions (fsn_train_*_chains), the committed fixture
(tests/golden/fsn_chain_grad_golden.npz, make_golden_fsn_chain_grad.py: every utterance ALONE at batch 1 on the genuine reference) and
the torch restatement of the chains contract (fsn_training.TrainableFullSubNet._torch_forward_chains, the checker of the kernels) in
float64 against it: per-utterance pred, exact zeros beyond every length, and the gradient of the batch loss sum_b sum(pred_b * R_b),
which is the sum of the three utterances' own gradients."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import FSN_TINY, ROOT, fsn_spec, rel_rms
from speech_enhancement_mi_amd import synth

# the cases of tests/golden/make_golden_fsn_chain.py / make_golden_fsn_chain_grad.py
SEED, TOTAL = 21, 12800
CALLS = (((False, False, False), (8000, 5200, 3400)), ((True, False, True), (4800, 7000, 3300)))
PAD = 3.0        # what the batches hold beyond each utterance's length: the forward must not read it
BAR = 1e-4       # relative RMS against the reference: the bar of test_fsn_training_cpu.py's gradient comparison
FIXTURE = os.path.join(ROOT, "tests", "golden", "fsn_chain_grad_golden.npz")
NEW = ("fsn_train_ws_bytes_chains", "fsn_train_fwd_chains", "fsn_train_bwd_chains")


def tiny_model():
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    m = TrainableFullSubNet(**FSN_TINY)
    sd = synth.make_state_dict(fsn_spec(FSN_TINY), seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def fixture_batch(call, pad=PAD):
    """The batch of call 0 / 1: [3, M, Lmax] with `pad` beyond each utterance's length; utterance b continues where its call-0 chunk ended"""
    mix = synth.synth_utterances(3, TOTAL, FSN_TINY["num_mics"], seed=SEED)[0]
    lens = CALLS[call][1]
    x = np.full((3, mix.shape[1], max(lens)), pad, np.float32)
    for b, L in enumerate(lens):
        lo = 0 if call == 0 else CALLS[0][1][b]
        x[b, :, :L] = mix[b, :, lo:lo + L]
    return torch.from_numpy(x)


def fixture_R(g, call):
    """R [3, Lmax] of the batch loss sum(pred * R): utterance b's recorded R, zeros beyond its length"""
    lens = CALLS[call][1]
    R = np.zeros((3, max(lens)), np.float32)
    for b, L in enumerate(lens):
        R[b, :L] = g[f"call{call + 1}_utt{b}_R"]
    return torch.from_numpy(R)


def fixture_gradsum(g, call, name):
    """the gradient of the batch loss of call 0 / 1: the sum over the utterances of the reference's own gradients"""
    if str(g["grad_layout"]) == "sum":
        return g[f"call{call + 1}_gradsum.{name}"]
    return sum(g[f"call{call + 1}_utt{b}_grad.{name}"].astype(np.float64) for b in range(3))


def test_abi_has_the_chain_training_entry_points():
    from speech_enhancement_mi_amd import engine
    lib = ctypes.CDLL(engine.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "se_engine.h")).read()
    for name in NEW:
        assert name in engine.EXPORTS, name
        assert hasattr(lib, name), name
        assert f" {name}(" in header, name
    assert all(n in header.split("additions at 5:")[1].split("*/")[0] for n in NEW)
    assert lib.se_abi_version() == 5


def test_fixture_is_committed_and_small():
    assert os.path.getsize(FIXTURE) <= 1024 * 1024
    g = np.load(FIXTURE)
    names = [k for k, _ in tiny_model().named_parameters()]
    for c in range(2):
        for b, L in enumerate(CALLS[c][1]):
            assert g[f"call{c + 1}_utt{b}_pred"].shape == (L,) and g[f"call{c + 1}_utt{b}_R"].shape == (L,)
        for k in names:
            assert np.abs(fixture_gradsum(g, c, k)).max() > 0, (c, k)


def test_restatement_vs_reference_chains():
    g = np.load(FIXTURE)
    m = tiny_model().double()
    for c, (flags, lens) in enumerate(CALLS):
        m.zero_grad(set_to_none=True)
        x = fixture_batch(c).double()
        pred, crm, s, xf = m.realtime_process(x, x.clone(), flag=list(flags), train=False, lengths=list(lens))
        assert pred.requires_grad and not crm.requires_grad and not s.requires_grad and not xf.requires_grad
        assert pred.shape == (3, max(lens)) and crm.shape[1:] == (3, 2, 201, 21) and s.shape == crm.shape and xf.shape == crm.shape
        Nb = [int(crm[:, b].flatten(1).abs().amax(dim=1).nonzero().max()) + 1 for b in range(3)]
        assert max(Nb) == crm.shape[0] and len(set(Nb)) > 1, Nb    # dead windows hold exact zeros, and there are some
        for b, L in enumerate(lens):
            e = rel_rms(pred[b, :L].detach().numpy(), g[f"call{c + 1}_utt{b}_pred"])
            assert e <= BAR, (c, b, e)
            assert bool((pred[b, L:] == 0).all()), (c, b)
        (pred * fixture_R(g, c).double()).sum().backward()
        for k, p in m.named_parameters():
            e = rel_rms(p.grad.numpy(), fixture_gradsum(g, c, k))
            assert e <= BAR, f"call {c + 1} {k}: rel rms {e:.2e}"


def test_uniform_list_is_the_scalar_call():
    mix, _ = synth.synth_utterances(2, 8000, 3, seed=7)
    outs = []
    for listed in (False, True):
        m = tiny_model()
        got = []
        for a, b, flag in ((0, 4800, False), (4800, 8000, True)):
            x = torch.from_numpy(mix[..., a:b].copy())
            kw = dict(flag=[flag, flag], lengths=[b - a, b - a]) if listed else dict(flag=flag)
            m.zero_grad(set_to_none=True)
            pred = m.realtime_process(x, train=False, **kw)
            pred.square().sum().backward()
            got += [pred.detach()] + [p.grad.clone() for p in m.parameters()]
        outs.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_chains_need_a_first_chunk_and_the_same_batch():
    m = tiny_model()
    x = fixture_batch(0)
    with pytest.raises(RuntimeError, match="flag=False"):
        m.realtime_process(x, flag=[True, False, True], train=False, lengths=list(CALLS[0][1]))
    with torch.no_grad():
        m.realtime_process(x, flag=[False] * 3, train=False, lengths=list(CALLS[0][1]))
        with pytest.raises(RuntimeError, match="holds 3 utterances, not 2"):
            m.realtime_process(x[:2], flag=[True, False], train=False, lengths=[4000, 3000])
