"""FullSubNet chunk-chain training step time: forward + full compute_loss + backward of TrainableFullSubNet.use_hip_kernels(True) at
FSN_FULL, timed with device events (median after warm-up), in two setups per step:

  chains : `--utts` ChunkChains served by datagen.ChunkChainBatch (chunk lengths drawn as data_c.py draws them, 1 .. 3.75 s, own flag
           per chain): per-utterance lengths and flags (fsn_train_*_chains).  Consecutive steps: step 0 is FRESH (all flags False: the
           batch is sorted by window count, the workspace packed), the later ones CARRIED (the batch keeps its slots: dense unless the
           counts happen to be non-increasing)
  uniform: the same number of utterances, all as long as the longest chunk of the same step, one flag (the scalar path:
           fsn_train_fwd / fsn_train_bwd, the launches the project had before the chains entry points)

Prints ms and workspace bytes for both, and sum Nb / (N * B), the share of the dense layout's windows that are alive.

    python profiles/fsn_chain_train_time.py [--utts 8] [--steps 3] [--iters 3] [--uniform-only]

--uniform-only runs the scalar setup alone: it needs nothing of the chains entry points, so the same file times a build without them."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.fsn_train_time import FSN_FULL  # noqa: E402


def median_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--uniform-only", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    from speech_enhancement_mi_amd.engine import chain_geometry
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    spec = synth.fsn_param_spec(201, 3, 512, 384, 2, 15, 0)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()}
    B, K = args.utts, FSN_FULL["segment_length"]

    def model():
        m = TrainableFullSubNet(**FSN_FULL)
        m.load_state_dict(sd)
        return m.cuda().use_hip_kernels(True)

    mc, mu = model(), model()   # the chains carry their state from step to step; the uniform batch starts afresh every time

    def utterances(seed):
        rng = np.random.default_rng(seed)

        def make():   # 8 .. 15 s of synthetic speech-like signal, cut by the chain
            L = int(rng.integers(8 * 16000, 15 * 16000))
            mix, clean = synth.synth_utterances(1, L, 3, seed=int(rng.integers(1 << 30)))
            return torch.from_numpy(mix[0]), torch.from_numpy(clean[0]), torch.from_numpy(mix[0] * 0), L
        return make

    batches = ChunkChainBatch([ChunkChain(utterances(b), rng=np.random.default_rng(1000 + b)) for b in range(B)])

    def step(m, x, src, ln, flag, lengths):
        m.zero_grad(set_to_none=True)
        pred, crm, s, xf = m.realtime_process(x, src, flag, train=False, **({} if lengths is None else dict(lengths=lengths)))
        m.compute_loss(src[:, 0], pred, xf, s, crm, ln)[0].backward()

    for s in range(args.steps):
        d = next(batches)
        x, ln = d["mix"].cuda(), d["length"].cuda()
        src = d["source"].cuda()
        if src.dim() == 2:
            src = src[:, None, :].repeat(1, 3, 1)
        Lmax = x.shape[-1]
        lens, flags = d["length"].tolist(), [bool(f) for f in d["flag"].tolist()]
        Nb = chain_geometry(lens, flags, K)["Nb"]
        Nu = chain_geometry([Lmax], [False], K)["Nb"][0]
        full = torch.full((B,), Lmax, dtype=torch.int64, device="cuda")
        mixu, cleanu = synth.synth_utterances(B, Lmax, 3, seed=50 + s)
        xu = torch.from_numpy(mixu).cuda()
        su = torch.from_numpy(np.repeat(cleanu[:, None, :], 3, axis=1).copy()).cuda()
        eng = mu._engine_for(xu)
        uniform = lambda: step(mu, xu, su, full, False, None)
        uniform()   # warm-up
        torch.cuda.synchronize()
        tu, wu = median_ms(uniform, args.iters), eng.train_ws_bytes(B, Nu)
        head = (f"step {s}: Lmax {Lmax} ({Lmax / 16000:.2f} s), flags {''.join('T' if f else 'F' for f in flags)}, windows {Nb} of {max(Nb)}, "
                f"sum Nb / (N B) {sum(Nb) / (max(Nb) * B):.2f}")
        if args.uniform_only:
            print(f"{head}: uniform {tu:.1f} ms, {wu / 2 ** 30:.2f} GiB")
            continue
        engc = mc._engine_for(x)
        # repetitions of a carried step continue whatever state the previous repetition left: the same launches, other numbers
        chains = lambda: step(mc, x, src, ln, flags, lens)
        chains()    # warm-up, and the state the next step continues
        torch.cuda.synchronize()
        order = engc._order if engc._order is not None else list(range(B))
        wc = engc.train_ws_bytes_chains(B, Lmax, [lens[i] for i in order], [flags[i] for i in order])
        tc = median_ms(chains, args.iters)
        print(f"{head}: chains {tc:.1f} ms, {wc / 2 ** 30:.2f} GiB; uniform at Lmax ({Nu} windows) {tu:.1f} ms, {wu / 2 ** 30:.2f} GiB; "
              f"time ratio {tc / tu:.3f}, workspace ratio {wc / wu:.3f}")


if __name__ == "__main__":
    main()
