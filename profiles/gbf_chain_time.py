"""GeneralBeamformer on a ragged batch of chunk chains (config.yaml geometry): inference, and forward + loss + backward on GBFFunction,
timed with device events after warm-up (median of `--iters`), two ways on this checkout:

  chains : `--utts` ChunkChains served by datagen.ChunkChainBatch (chunk lengths 1 .. 3.75 s as data_c.py draws them): per-utterance
           lengths, the persistent GRU with per-stream step counts; every step of `--steps` is a different batch, all flags reset
  padded : the same batch padded to Lmax through the uniform call (one length, one flag)

and, with `--root DIR` (another checkout of this repository with its library built, e.g. a worktree of the parent commit), the padded
batch through THAT checkout's uniform call only.  The share of the persistent GRU launches in each is printed from the per-kernel
events of train_ops.PROF.  The U-Net and the head kernels still run the dead segments, so only the GRU part shrinks.

    python profiles/gbf_chain_time.py [--utts 8] [--steps 4] [--iters 3] [--root DIR]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(num_channels=[128, 128, 128, 128], num_freqs=201, hidden=256, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3,
            dropout=0.0, sample_rate=16000, win_length=25, hop_length=10, n_fft=400)   # config.yaml:233-245


def ev_ms(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--root", default=None, help="time the padded batch on the package of this checkout instead (uniform call only)")
    args = ap.parse_args()
    other = args.root is not None
    sys.path.insert(0, os.path.abspath(args.root) if other else HERE)
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer
    print("package:", os.path.dirname(os.path.abspath(synth.__file__)))
    spec = synth.gbf_param_spec(FULL["num_channels"], FULL["num_freqs"], FULL["hidden"], FULL["segment_length"], FULL["num_layers"], 3, 3)
    m = GeneralBeamformer(**FULL).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()}, strict=True)
    m = m.cuda().use_hip_training(True)
    B = args.utts

    def utterances(seed):
        rng = np.random.default_rng(seed)

        def make():   # 8 .. 15 s of synthetic speech-like signal, cut by the chain
            L = int(rng.integers(8 * 16000, 15 * 16000))
            mix, clean = synth.synth_utterances(1, L, 3, seed=int(rng.integers(1 << 30)))
            return torch.from_numpy(mix[0]), torch.from_numpy(clean[0]), torch.from_numpy(mix[0] * 0), L
        return make

    batches = ChunkChainBatch([ChunkChain(utterances(b), rng=np.random.default_rng(1000 + b)) for b in range(B)])

    def infer(x, lengths):
        with torch.no_grad():
            m.realtime_process(x, False) if lengths is None else m.realtime_process(x, False, lengths=lengths)

    def train(x, src, ln, lengths):
        m.zero_grad(set_to_none=True)
        pred = m.realtime_process(x, False) if lengths is None else m.realtime_process(x, False, lengths=lengths)
        m.compute_loss(src, pred, ln)[0].backward()

    def timed(fn):
        fn()   # warm-up
        torch.cuda.synchronize()
        ms = ev_ms(fn, args.iters)
        K.PROF = {}
        fn()
        prof = K.profile_summary()
        K.PROF = None
        gru = sum(v["ms"] for k, v in prof.items() if k.startswith("k_gru_pseq"))
        return ms, gru / max(sum(v["ms"] for v in prof.values()), 1e-9)

    names = ["padded"] if other else ["chains", "padded"]
    tot = {(w, n): [0.0, 0.0] for w in ("inference", "training") for n in names}
    ratios = []
    for s in range(args.steps):
        d = next(batches)
        x, src, ln = d["mix"].cuda(), d["source"].cuda(), d["length"].cuda()
        Lmax, lens = x.shape[-1], d["length"].tolist()
        ratios.append(float(d["length"].float().mean()) / Lmax)
        line = [f"step {s}: Lmax {Lmax} ({Lmax / 16000:.2f} s), mean / max length {ratios[-1]:.2f}:"]
        for n in names:
            lengths = lens if n == "chains" else None
            for w, fn in (("inference", lambda: infer(x, lengths)), ("training", lambda: train(x, src, ln, lengths))):
                ms, share = timed(fn)
                tot[(w, n)][0] += ms
                tot[(w, n)][1] += share
                line.append(f"{w} {n} {ms:.1f} ms (GRU {100 * share:.0f} %)")
        print(" ".join(line), flush=True)
    print(f"{B} utterances, {args.steps} steps, mean / max length {sum(ratios) / len(ratios):.2f}")
    for (w, n), (ms, share) in tot.items():
        print(f"  {w:9s} {n:7s}: {ms / args.steps:7.1f} ms per call, persistent GRU launches {100 * share / args.steps:.0f} % of the kernel time")


if __name__ == "__main__":
    main()
