"""HiFi-GAN generator inference on a ragged batch of chunk chains (hash weights, Hifi-GAN/config.yaml's geometry: channels
[16, 32, 64, 128], hidden 512, two LSTM layers), timed with device events after a warm-up of every shape (median of `--iters`), two ways:

  chains : `--utts` ChunkChains served by datagen.ChunkChainBatch (chunk lengths 1 .. 3.75 s as data_c.py draws them) as ONE
           realtime_process_chains call with per-stream lengths: the streams sorted by window count, every pass on the prefix still
           running (call_plan.chain_passes), the LSTM and the norm's scan per stream; every step of `--steps` is a different batch, all reset
  padded : the same batches padded to Lmax through realtime_process (one length, one reset)

Next to the times: the share of (stream, window) pairs that are some stream's own, and the share the chains call runs - live windows
rounded up to a pass of max_segments windows.  The LSTM is one launch per time step and its step count follows the longest stream in
either form, so the chains call saves on the convolutions and the postnet only.

Each of the two measurements runs in a child process of its own under `timeout`, one after the other, and the first one that fails
ends the run:

    python profiles/hifigan_chain_time.py [--utts 8] [--steps 4] [--iters 10] [--max-segments 8] [--limit 240]"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FULL = dict(num_channels=[16, 32, 64, 128], num_freqs=201, hidden=512, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3, dropout=0.0,
            sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(name, args):
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.call_plan import chain_geometry
    from speech_enhancement_mi_amd.datagen import ChunkChain, ChunkChainBatch
    from speech_enhancement_mi_amd.hifigan import Generator
    spec = synth.hifigan_param_spec(FULL["num_channels"], FULL["num_freqs"], FULL["hidden"], FULL["num_layers"], FULL["num_inputs"], FULL["kernel_size"])
    m = Generator(**FULL).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hifigan_state_dict(spec, seed=0).items()}, strict=True)
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
    total = 0.0
    with torch.no_grad():
        for s in range(args.steps):
            d = next(batches)
            x, lens = d["mix"].cuda(), d["length"].tolist()
            Lmax = x.shape[-1]

            def call():
                m.reset_norm()
                return m.realtime_process_chains(x, True, lens) if name == "chains" else m.realtime_process(x, reset=True)
            call()                                       # warm-up of this shape
            torch.cuda.synchronize()
            ts = sorted(ev_ms(call) for _ in range(args.iters))
            Nb = chain_geometry(lens, [False] * B, FULL["segment_length"])["Nb"]
            N = max(Nb)
            run = sum(min(step, N - n0) * sum(nb > n0 for nb in Nb) for n0 in range(0, N, step))
            total += ts[len(ts) // 2]
            print(f"  {name} step {s}: Lmax {Lmax} ({Lmax / 16000:.2f} s), {N} windows, own (stream, window) pairs {sum(Nb) / (N * B):.2f}, run by the "
                  f"chains call {run / (N * B):.2f}: {ts[len(ts) // 2]:.1f} ms (min {ts[0]:.1f}, max {ts[-1]:.1f}), passes {m._last_passes}", flush=True)
    print(f"{name:7s}: {total / args.steps:8.1f} ms per call ({B} streams, {args.steps} steps, max_segments {step}, median of {args.iters} calls each, "
          f"{torch.cuda.get_device_name(0)})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-segments", type=int, default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one measurement")
    ap.add_argument("--child", choices=["chains", "padded"], help="run one measurement in this process")
    args = ap.parse_args()
    if args.child:
        measure(args.child, args)
        return 0
    passed = ["--utts", str(args.utts), "--steps", str(args.steps), "--iters", str(args.iters)] + (["--max-segments", str(args.max_segments)] if args.max_segments else [])
    for name in ("chains", "padded"):
        rc = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", name] + passed).returncode
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"{name}: exit status {rc}, stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
