"""The chunk-chain cases of tests/golden/make_golden_chain.py, shared by test_chain_cpu.py and test_gpu_chain_training.py: three
utterances, two calls, per-utterance lengths and flags; the fixture holds what the genuine reference gives for each utterance ALONE."""
import os

import numpy as np
import torch

from conftest import ROOT, TINY, spec_of_variant
from speech_enhancement_mi_amd import synth

SEED, TOTAL = 21, 12800
CALLS = (((False, False, False), (8000, 5200, 3400)), ((True, False, True), (4800, 7000, 3300)))
VARIANTS = (("crn", 0), ("elu", 1), ("student", 2))
PAD = 3.0   # what the batches hold beyond each utterance's length: the forward must not read it


def chain_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "crn_chain_golden.npz"))


def tiny_model(variant, seed=0):
    from speech_enhancement_mi_amd.training import TrainableCRN, TrainableCRNELU, TrainableStudentCRN
    m = (TrainableCRN, TrainableCRNELU, TrainableStudentCRN)[variant](**TINY)
    sd = synth.make_state_dict(spec_of_variant(TINY, variant), seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def chain_batch(call, mix=None, calls=CALLS, pad=PAD):
    """The batch of call 0 / 1: [B, M, Lmax] with `pad` beyond each utterance's length; utterance b continues where its call-0 chunk ended"""
    if mix is None:
        mix = synth.synth_utterances(len(calls[0][1]), TOTAL, TINY["num_inputs"], seed=SEED)[0]
    lens = calls[call][1]
    x = np.full((mix.shape[0], mix.shape[1], max(lens)), pad, np.float32)
    for b, L in enumerate(lens):
        lo = 0 if call == 0 else calls[0][1][b]
        x[b, :, :L] = mix[b, :, lo:lo + L]
    return torch.from_numpy(x)
