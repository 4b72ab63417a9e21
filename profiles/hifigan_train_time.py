"""HiFi-GAN generator training time (Hifi-GAN/config.yaml geometry): forward + Hifi_GAN.train_stage(stage=2) loss + backward on B
utterances x 3 s, Generator.use_hip_training(True) (hifigan_training.HifiFunction) against the torch fp32 restatement on the same GPU,
timed with device events after warm-up (median of --iters with min - max), peak device memory of each, and the kernel path's per-kernel
split from train_ops.profile_summary() (one further step with an event pair around every launch, so it is not part of the timing).

    python profiles/hifigan_train_time.py [--utts 1 2 8] [--seconds 3] [--iters 5] [--no-torch] [--max-segments 8]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FULL = dict(num_channels=[16, 32, 64, 128], num_freqs=201, hidden=512, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3, dropout=0.0,
            sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--max-segments", type=int, default=8)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.hifigan import Hifi_GAN
    c = FULL
    spec = synth.hifigan_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["num_layers"], c["num_inputs"], c["kernel_size"])
    sd = {k: torch.from_numpy(v) for k, v in synth.hifigan_state_dict(spec, seed=0).items()}
    L = int(args.seconds * 16000)

    def timed(hip, B, iters):
        mix, clean = synth.synth_utterances(B, L, 3, seed=11)
        x, y = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
        y = y if y.dim() == 2 else y[:, 0]
        w = Hifi_GAN([], [], **c)
        w.generator.load_state_dict(sd)
        w = w.cuda().eval()
        w.generator.max_segments = args.max_segments
        w.generator.use_hip_training(True) if hip else w.generator.use_hip_kernels(False)

        def step():
            loss = w.train_stage(x, y, stage=2, reset=True)
            loss.backward()
            w.zero_grad(set_to_none=True)
        step()  # warm-up: library load, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        split = None
        if hip:
            K.PROF = {}
            step()
            split = K.profile_summary()
            K.PROF = None
        del w
        torch.cuda.empty_cache()
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), peak, split

    print(f"HiFi-GAN generator training step (forward + stage-2 stft_loss + backward), {args.seconds:g} s utterances, max_segments "
          f"{args.max_segments}, {torch.cuda.get_device_name(0)}")
    for B in args.utts:
        med, lo, hi, mem, split = timed(True, B, args.iters)
        line = f"B = {B}: HIP kernels {med:9.1f} ms ({lo:.1f} - {hi:.1f}), peak {mem:6.2f} GiB, {B * 1000.0 / med:6.2f} utt/s"
        if not args.no_torch:
            t_med, t_lo, t_hi, t_mem, _ = timed(False, B, args.iters)
            line += f" | torch fp32 restatement {t_med:9.1f} ms ({t_lo:.1f} - {t_hi:.1f}), peak {t_mem:6.2f} GiB | speed-up {t_med / med:5.2f}x"
        print(line, flush=True)
        total = sum(v["ms"] for v in split.values())
        for k, v in sorted(split.items(), key=lambda kv: -kv[1]["ms"]):
            print(f"    {k:24s} {v['ms']:9.2f} ms {100.0 * v['ms'] / total:5.1f} %  {v['launches']:5d} launches", flush=True)


if __name__ == "__main__":
    main()
