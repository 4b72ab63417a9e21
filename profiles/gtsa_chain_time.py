"""GTSA inference on a ragged batch of chunk chains (full fixture geometry: 6 layers, fn_dim 1024, maxlen 210), timed with device events
after a warm-up of every shape (median of `--iters`, the two calls alternating), two ways on this checkout:

  chains : `--utts` ChunkChains served by datagen.ChunkChainBatch (chunk lengths 1 .. 3.75 s as data_c.py draws them) as ONE call with
           per-utterance lengths: the streams sorted by window count, every pass on the prefix still running (call_plan.chain_passes); every
           step of `--steps` is a different batch, all flags reset
  padded : the same batch padded to Lmax through the uniform call (one length, one flag)

and, with `--root DIR` (another checkout of this repository with its library built, e.g. a worktree of the parent commit), the padded
batch through THAT checkout's uniform call only.  Next to the times: the share of (stream, window) pairs that are some stream's own,
and the share the chains call runs - live windows rounded up to a pass of max_segments windows, which is what its cost should follow.
The chains output is compared with the padded one on every utterance's own samples (the arithmetic of a stream does not depend on
the batch, so the difference is expected to be exactly zero).

    python profiles/gtsa_chain_time.py [--utts 8] [--steps 4] [--iters 10] [--max-segments 8] [--root DIR]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = dict(num_mics=3, num_freqs=201, segment_length=3200, num_layers=6, num_heads=5, model_dim=201, fn_dim=1024, maxlen=210, dropout=0.0,
            sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-segments", type=int, default=None)
    ap.add_argument("--root", default=None, help="time the padded batch on the package of this checkout instead (uniform call only)")
    args = ap.parse_args()
    other = args.root is not None
    sys.path.insert(0, os.path.abspath(args.root) if other else HERE)
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.call_plan import chain_geometry
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    from speech_enhancement_mi_amd.gtsa import GTSA
    print("package:", os.path.dirname(os.path.abspath(synth.__file__)), "on", torch.cuda.get_device_name(0))
    spec = synth.gtsa_param_spec(FULL["num_mics"], FULL["num_freqs"], FULL["num_layers"], FULL["fn_dim"], FULL["maxlen"])
    m = GTSA(**FULL).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.gtsa_state_dict(spec, seed=0).items()}, strict=True)
    m = m.cuda()
    if args.max_segments:
        m.max_segments = args.max_segments
    B, step = args.utts, max(1, int(m.max_segments))

    def utterances(seed):
        rng = np.random.default_rng(seed)

        def make():   # 8 .. 15 s of synthetic speech-like signal, cut by the chain
            L = int(rng.integers(8 * 16000, 15 * 16000))
            mix, clean = synth.synth_utterances(1, L, 3, seed=int(rng.integers(1 << 30)))
            return torch.from_numpy(mix[0]), torch.from_numpy(clean[0]), torch.from_numpy(mix[0] * 0), L
        return make

    batches = ChunkChainBatch([ChunkChain(utterances(b), rng=np.random.default_rng(1000 + b)) for b in range(B)])
    names = ["padded"] if other else ["chains", "padded"]
    tot = {n: 0.0 for n in names}
    with torch.no_grad():
        for s in range(args.steps):
            d = next(batches)
            x, lens = d["mix"].cuda(), d["length"].tolist()
            Lmax = x.shape[-1]
            calls = dict(chains=lambda: m.realtime_process(x, False, lengths=lens), padded=lambda: m.realtime_process(x, False))
            ys = {n: calls[n]() for n in names}      # warm-up of both shapes
            torch.cuda.synchronize()
            ts = {n: [] for n in names}
            for _ in range(args.iters):              # alternating, so a drift of the machine hits both alike
                for n in names:
                    ts[n].append(ev_ms(calls[n]))
            Nb = chain_geometry(lens, [False] * B, FULL["segment_length"])["Nb"]
            N = max(Nb)
            run = sum(min(step, N - n0) * sum(nb > n0 for nb in Nb) for n0 in range(0, N, step))
            line = [f"step {s}: Lmax {Lmax} ({Lmax / 16000:.2f} s), {N} windows, own (stream, window) pairs {sum(Nb) / (N * B):.2f}, "
                    f"run by the chains call {run / (N * B):.2f}:"]
            for n in names:
                tot[n] += median(ts[n])
                line.append(f"{n} {median(ts[n]):.1f} ms (min {min(ts[n]):.1f}, max {max(ts[n]):.1f})")
            if not other:
                diff = max(float((ys["chains"][b, :L] - ys["padded"][b, :L]).abs().max()) for b, L in enumerate(lens))
                line.append(f"max |chains - padded| on own samples {diff:.1e}")
            print(" ".join(line), flush=True)
    print(f"{B} utterances, {args.steps} steps, max_segments {step}, median of {args.iters} calls each")
    for n in names:
        print(f"  {n:7s}: {tot[n] / args.steps:8.1f} ms per call")


if __name__ == "__main__":
    main()
