"""HiFi-GAN generator training time on a ragged batch of chunk chains (Hifi-GAN/config.yaml geometry, hash weights): forward +
Hifi_GAN stage-2 loss + backward on `--utts` chunks of 1 .. 3.75 s (seeded lengths, every stream reset), timed with device events after
a warm-up step (median of `--iters` with min - max) and with the peak device memory, three ways:

  chains      : Generator.use_hip_training(True, chains=True), Hifi_GAN.train_stage_chains with the per-stream lengths: ONE
                HifiFunction node on the sorted-prefix schedule, dead windows carrying a zero cotangent
  padded      : the same batch padded to Lmax through the uniform node, use_hip_training(True) and Hifi_GAN.train_stage - the only
                kernel route without chains=True (its loss is the whole-batch form and reads the padding: the time is what compares)
  restatement : use_hip_kernels(False), train_stage_chains: every stream alone at B = 1 on torch

Each leg runs in a child process of its own under `timeout`, one after the other, and the first one that fails ends the run:

    python profiles/hifigan_chain_train_time.py [--utts 8] [--iters 5] [--max-segments 8] [--limit 240] [--legs chains padded restatement]"""
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
LEGS = ("chains", "padded", "restatement")


def measure(name, args):
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.call_plan import chain_geometry
    from speech_enhancement_mi_amd.hifigan import Hifi_GAN
    c, B = FULL, args.utts
    spec = synth.hifigan_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["num_layers"], c["num_inputs"], c["kernel_size"])
    w = Hifi_GAN([], [], **c)
    w.generator.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hifigan_state_dict(spec, seed=0).items()})
    w = w.cuda().eval()
    g = w.generator
    g.max_segments = args.max_segments
    lens = [int(v) for v in np.random.default_rng(7).integers(16000, 60001, size=B)]   # 1 .. 3.75 s
    Lmax = max(lens)
    mix, clean = synth.synth_utterances(B, Lmax, 3, seed=11)
    clean = clean if clean.ndim == 2 else clean[:, 0]
    for b, L in enumerate(lens):
        mix[b, :, L:], clean[b, L:] = 0.0, 0.0
    x, y = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
    if name == "chains":
        g.use_hip_training(True, chains=True)
    elif name == "padded":
        g.use_hip_training(True)
    else:
        g.use_hip_kernels(False)

    def step():
        g.reset_norm()
        loss = w.train_stage(x, y, stage=2, reset=True) if name == "padded" else w.train_stage_chains(x, y, True, lens, stage=2)
        loss.backward()
        w.zero_grad(set_to_none=True)
    step()   # warm-up: library load, allocator
    torch.cuda.synchronize()
    assert g._last_path == ("torch" if name == "restatement" else "kernel")
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    Nb = chain_geometry(lens, [False] * B, c["segment_length"])["Nb"]
    print(f"{name:11s}: {np.median(ts):8.1f} ms ({min(ts):.1f} - {max(ts):.1f}), peak {torch.cuda.max_memory_allocated() / 2 ** 30:5.2f} GiB | {B} chunks of "
          f"{min(lens) / 16000:.2f} .. {Lmax / 16000:.2f} s, windows {Nb}, own (stream, window) pairs {sum(Nb) / (max(Nb) * B):.2f}, max_segments "
          f"{args.max_segments}, passes {g._last_passes}, median of {args.iters}, {torch.cuda.get_device_name(0)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-segments", type=int, default=8)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one leg")
    ap.add_argument("--legs", nargs="+", choices=LEGS, default=list(LEGS))
    ap.add_argument("--child", choices=LEGS, help="run one leg in this process")
    args = ap.parse_args()
    if args.child:
        measure(args.child, args)
        return 0
    passed = ["--utts", str(args.utts), "--iters", str(args.iters), "--max-segments", str(args.max_segments)]
    for name in args.legs:
        rc = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", name] + passed).returncode
        if rc != 0:   # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"{name}: exit status {rc}, stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
