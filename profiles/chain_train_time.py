"""Batched chunk-chain training step time: forward + full loss (0.7 STOI + 0.3 -SI-SNR) + backward of the FULL400 CRN on the kernels,
timed with device events after warm-up, in two setups:

  chains : `--utts` ChunkChains served by datagen.ChunkChainBatch (chunk lengths drawn as data_c.py draws them, 1 .. 3.75 s, own flag
           per chain): per-utterance lengths and flags, the row kernels; every step of `--steps` is a different batch
  uniform: the same number of utterances, all as long as the longest chunk of the same step (the batch the scalar kernels take)

Dead segments (past an utterance's end) still run, so the two are expected to cost about the same; the mean / max length ratio of each
step says how much of the ragged batch is padding.

    python profiles/chain_train_time.py [--utts 8] [--steps 6] [--iters 3]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.distill_train_time import FULL400, ev_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    from speech_enhancement_mi_amd.training import TrainableCRN
    c = FULL400
    spec = synth.crn_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["num_layers"], 3, 3)
    m = TrainableCRN(**c)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()})
    m = m.cuda().use_hip_kernels(True)
    B = args.utts

    def utterances(seed):
        rng = np.random.default_rng(seed)

        def make():   # 8 .. 15 s of synthetic speech-like signal, cut by the chain
            L = int(rng.integers(8 * 16000, 15 * 16000))
            mix, clean = synth.synth_utterances(1, L, 3, seed=int(rng.integers(1 << 30)))
            return torch.from_numpy(mix[0]), torch.from_numpy(clean[0]), torch.from_numpy(mix[0] * 0), L
        return make

    batches = ChunkChainBatch([ChunkChain(utterances(b), rng=np.random.default_rng(1000 + b)) for b in range(B)])

    def step(x, src, ln, flag, lengths):
        m.zero_grad(set_to_none=True)
        pred = m.realtime_process_train(x, flag, lengths=lengths)
        m.compute_loss(src, pred, ln)[0].backward()

    tot = dict(chains=0.0, uniform=0.0)
    ratios = []
    for s in range(args.steps):
        d = next(batches)
        x, src, ln = d["mix"].cuda(), d["source"].cuda(), d["length"].cuda()
        Lmax = x.shape[-1]
        ratio = float(d["length"].float().mean()) / Lmax
        ratios.append(ratio)
        lens, flags = d["length"].tolist(), d["flag"].tolist()
        full = torch.full((B,), Lmax, dtype=torch.int64, device="cuda")
        xu = torch.from_numpy(synth.synth_utterances(B, Lmax, 3, seed=50 + s)[0]).cuda()
        su = torch.from_numpy(synth.synth_utterances(B, Lmax, 3, seed=50 + s)[1]).cuda()
        state = m._state

        def chains():
            m._state = state   # every repetition continues the same carried state
            step(x, src, ln, flags, lens)

        def uniform():
            step(xu, su, full, False, None)
        chains(), uniform()   # warm-up
        torch.cuda.synchronize()
        tc, tu = ev_ms(chains, args.iters), ev_ms(uniform, args.iters)
        chains()              # leave the chains' own state behind for the next step
        tot["chains"] += tc
        tot["uniform"] += tu
        print(f"step {s}: Lmax {Lmax} ({Lmax / 16000:.2f} s), mean / max length {ratio:.2f}, flags {''.join('T' if f else 'F' for f in flags)}: "
              f"chains {tc:.1f} ms, uniform {tu:.1f} ms")
    print(f"{B} utterances, {args.steps} steps: chains {tot['chains'] / args.steps:.1f} ms per step, uniform at Lmax {tot['uniform'] / args.steps:.1f} ms per step, "
          f"ratio {tot['chains'] / tot['uniform']:.3f}; mean / max length {sum(ratios) / len(ratios):.2f}")


if __name__ == "__main__":
    main()
