"""Batched chunk-chain training, CPU side: the per-utterance geometry, the batched chain loader, the torch restatement path with
per-utterance lengths and flags against what the genuine reference gives for every utterance alone (tests/golden/crn_chain_golden.npz,
tests/golden/make_golden_chain.py), and the C ABI declarations of the row kernels."""
import os
import re

import numpy as np
import pytest
import torch

from chain_cases import CALLS, VARIANTS, chain_batch, chain_golden, tiny_model
from conftest import ROOT, rel_rms


def test_ragged_geometry_is_segment_geometry_per_utterance():
    from speech_enhancement_mi_amd.train_stages import ragged_geometry, segment_geometry
    rng = np.random.default_rng(0)
    lengths = [1, 799, 1599, 1600, 1601, 3199, 3200, 3201, 4800, 4801, 16000, 59999] + [int(v) for v in rng.integers(1, 60000, 40)]
    flags = [bool(v) for v in rng.integers(0, 2, len(lengths))]
    for Ks, hop, n_fft in ((3200, 160, 400), (3200, 160, 512), (1600, 160, 400)):
        q = ragged_geometry(lengths, flags, Ks, hop, n_fft, [5, 16, 32])
        per = [segment_geometry(L, f, Ks, hop, n_fft, [5, 16, 32]) for L, f in zip(lengths, flags)]
        for key, mine in (("Lp", "Lp"), ("gap", "gap"), ("N", "Nb"), ("off0", "off0"), ("skip", "skip"), ("L", "lengths")):
            assert q[mine] == [p[key] for p in per], key
        assert q["N"] == max(p["N"] for p in per) and q["L"] == max(lengths)
        assert all(q[k] == per[0][k] for k in ("Ks", "P", "T", "F0", "ch", "Fq"))
        assert min(q["Nb"]) >= 2 and all(n % 2 == 0 for n in q["Nb"])
    for f in (False, True):   # one utterance: the scalar geometry
        q, p = ragged_geometry([5000], [f], 3200, 160, 400), segment_geometry(5000, f, 3200, 160, 400)
        assert (q["N"], q["off0"], q["skip"], q["gap"]) == (p["N"], [p["off0"]], [p["skip"]], [p["gap"]])


def test_as_flags_keeps_a_mixed_tensor_mixed():
    from speech_enhancement_mi_amd.train_stages import _as_flags, _as_lengths
    assert _as_flags(torch.tensor([True, False, True]), 3) == [True, False, True]
    assert _as_flags([0, 1], 2) == [False, True] and _as_flags(True, 2) == [True, True] and _as_flags(torch.tensor(False), 1) == [False]
    assert _as_flags(torch.tensor([True]), 2) == [True, True]   # the reference trainer's one flag per batch
    with pytest.raises(ValueError):
        _as_flags([True, False, True], 2)
    assert _as_lengths(None, 2, 7) == [7, 7] and _as_lengths(torch.tensor([3, 7]), 2, 7) == [3, 7]
    for bad in ([3], [3, 8], [0, 7]):
        with pytest.raises(ValueError):
            _as_lengths(bad, 2, 7)


def _utterances(seed, M=3):
    rng = np.random.default_rng(seed)

    def make():
        L = int(rng.integers(30000, 130000))
        x = rng.standard_normal((M, L)).astype(np.float32)
        return torch.from_numpy(x), torch.from_numpy(x[0] * 0.5), torch.from_numpy(x * 0.25), L
    return make


def test_chunk_chain_batch_serves_every_chain_its_own_chunks():
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    B = 4
    batch = ChunkChainBatch([ChunkChain(_utterances(10 + b), rng=np.random.default_rng(100 + b)) for b in range(B)])
    alone = [ChunkChain(_utterances(10 + b), rng=np.random.default_rng(100 + b)) for b in range(B)]
    seen = set()
    for _ in range(12):
        d = next(batch)
        ref = [next(c) for c in alone]
        Lmax = max(r["length"] for r in ref)
        assert d["mix"].shape == (B, 3, Lmax) and d["source"].shape == (B, Lmax) and d["noise"].shape == (B, 3, Lmax)
        assert d["length"].dtype == torch.int64 and d["flag"].dtype == torch.bool
        assert d["length"].tolist() == [r["length"] for r in ref] and d["flag"].tolist() == [r["flag"] for r in ref]
        for b, r in enumerate(ref):
            L = r["length"]
            for key in ("mix", "source", "noise"):
                assert torch.equal(d[key][b, ..., :L], r[key]) and not d[key][b, ..., L:].any()
        seen.add(tuple(d["flag"].tolist()))
    assert any(len(set(f)) > 1 for f in seen), "the case must contain a step with mixed flags"


@pytest.mark.parametrize("tag,variant", VARIANTS)
def test_restatement_path_batched_chains_match_the_reference_per_utterance(tag, variant):
    """Three utterances with their own lengths and flags in ONE batch, two calls, on the torch restatement: every utterance equals the
    genuine reference run on it alone (1e-4 relative RMS, the project's parity bar); nothing beyond an utterance's length."""
    g = chain_golden()
    m = tiny_model(variant)
    with torch.no_grad():
        for c, (flags, lens) in enumerate(CALLS):
            flag = torch.tensor(flags) if c else list(flags)
            pred = m.realtime_process_train(chain_batch(c), flag, lengths=torch.tensor(lens) if c else list(lens))
            assert pred.shape == (3, max(lens))
            for b, L in enumerate(lens):
                err = rel_rms(pred[b, :L].numpy(), g[f"{tag}_call{c + 1}_utt{b}"])
                print(f"{tag} call {c + 1} utterance {b}: rel rms {err:.2e}")
                assert err < 1e-4, (tag, c, b, err)
                assert not pred[b, L:].any()


def test_mixed_flags_are_not_collapsed():
    """flag [T, F, T] differs from both uniform readings of it on the utterance that disagrees"""
    m = tiny_model(0)
    outs = {}
    with torch.no_grad():
        for name, flag2 in (("mixed", [True, False, True]), ("all", True)):
            m._state = None
            m.realtime_process_train(chain_batch(0), False, lengths=list(CALLS[0][1]))
            outs[name] = m.realtime_process_train(chain_batch(1), flag2, lengths=list(CALLS[1][1]))
    L = CALLS[1][1]
    assert torch.equal(outs["mixed"][0, :L[0]], outs["all"][0, :L[0]]) and torch.equal(outs["mixed"][2, :L[2]], outs["all"][2, :L[2]])
    assert rel_rms(outs["mixed"][1, :L[1]].numpy(), outs["all"][1, :L[1]].numpy()) > 1e-3


def test_continuation_needs_a_carried_batch_of_the_same_size():
    m = tiny_model(0)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            m.realtime_process_train(chain_batch(1), [True, False, True], lengths=list(CALLS[1][1]))
        m.realtime_process_train(chain_batch(0)[:2], False, lengths=list(CALLS[0][1][:2]))
        with pytest.raises(RuntimeError):
            m.realtime_process_train(chain_batch(1), [True, False, True], lengths=list(CALLS[1][1]))


def test_train_step_takes_flag_and_length():
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.training import FlatBucket, train_step
    _, clean = synth.synth_utterances(3, 8000, 3, seed=5)
    res = []
    for pad in (3.0, -5.0):   # what lies beyond the lengths does not reach the gradient
        m = tiny_model(0)
        bucket = FlatBucket(list(m.parameters()))
        opt = torch.optim.Adam(m.parameters(), lr=3e-4)
        l1 = train_step(m, bucket, opt, chain_batch(0, pad=pad), torch.from_numpy(clean), torch.tensor(CALLS[0][1]), flag=torch.tensor(CALLS[0][0]))
        l2 = train_step(m, bucket, opt, chain_batch(1, pad=pad), torch.from_numpy(clean[:, :7000]), torch.tensor(CALLS[1][1]), flag=torch.tensor(CALLS[1][0]))
        assert np.isfinite(l1) and np.isfinite(l2) and float(bucket.flat.abs().sum()) > 0
        res.append((l1, l2, bucket.flat.clone()))
    assert res[0][:2] == res[1][:2] and torch.equal(res[0][2], res[1][2])


def test_row_kernels_are_declared_in_the_header():
    text = open(os.path.join(ROOT, "include", "se_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    from speech_enhancement_mi_amd import engine
    for name in ("se_sig_stft_rows", "se_train_ola_fwd_rows", "se_train_ola_bwd_rows", "se_train_slab_gather"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in engine.EXPORTS
    assert re.search(r"se_sig_stft_rows\s*\(\s*se_sig \*g, const float \*wav, int B, int M, int64_t Lmax, const int64_t \*off0, const int64_t \*len,", text)
