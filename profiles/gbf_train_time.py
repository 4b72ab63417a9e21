"""GeneralBeamformer training time (config.yaml:233-245): forward + compute_loss + backward of realtime_process on B utterances x 3 s,
GeneralBeamformer.use_hip_training(True) (general_beamformer.GBFFunction) against the torch fp32 restatement on the same GPU, timed
with device events after warm-up; peak device memory of each.

    python profiles/gbf_train_time.py [--utts 1 2 8] [--seconds 3] [--iters 3] [--no-torch]

Kernel split: run it under `rocprofv3 --kernel-trace --stats -- python profiles/gbf_train_time.py --no-torch`."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GBF_FULL = dict(num_channels=[128, 128, 128, 128], num_freqs=201, hidden=256, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3,
                dropout=0.0, sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer
    c = GBF_FULL
    spec = synth.gbf_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["segment_length"], c["num_layers"], c["num_inputs"],
                                c["kernel_size"])
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()}
    L = int(args.seconds * 16000)

    def timed(hip, B, iters):
        mix, clean = synth.synth_utterances(B, L, 3, seed=11)
        x, src = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
        lens = torch.full((B,), L, dtype=torch.int64, device="cuda")
        m = GeneralBeamformer(**c)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        m.use_hip_training(True) if hip else m.use_hip_kernels(False)

        def step():
            pred = m.realtime_process(x, torch.zeros(B, dtype=torch.bool))
            loss = m.compute_loss(src, pred, lens)[0]
            loss.backward()
            m.zero_grad(set_to_none=True)
        step()  # warm-up: library load, workspace allocation
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
        del m
        torch.cuda.empty_cache()
        return float(np.median(ts)), float(np.min(ts)), peak

    print(f"GeneralBeamformer training step (forward + compute_loss + backward), {args.seconds:g} s utterances, "
          f"{torch.cuda.get_device_name(0)}")
    for B in args.utts:
        h_med, h_min, h_mem = timed(True, B, args.iters)
        line = f"B = {B}: HIP kernels {h_med:9.1f} ms (min {h_min:.1f}), peak {h_mem:6.2f} GiB, {B * 1000.0 / h_med:6.2f} utt/s"
        if not args.no_torch:
            t_med, t_min, t_mem = timed(False, B, args.iters)
            line += f" | torch fp32 restatement {t_med:9.1f} ms (min {t_min:.1f}), peak {t_mem:6.2f} GiB | speed-up {t_med / h_med:5.2f}x"
        print(line, flush=True)


if __name__ == "__main__":
    main()
