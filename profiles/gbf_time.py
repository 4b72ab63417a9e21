"""GeneralBeamformer inference time (config.yaml geometry, hash weights): realtime_process of B utterances x 3 s, flag=False, under
no_grad.  For each batch size: the kernel path and the torch restatement on the same GPU (median ms over --iters after one warm-up,
real-time factor = seconds of audio processed per second / batch, peak torch.cuda.max_memory_allocated), then a per-stage breakdown
of one kernel-path call through train_ops.PROF, and the kernel path at other max_segments values.

    python profiles/gbf_time.py [--batches 1 8 64] [--seconds 3] [--iters 3] [--no-torch] [--max-segments 1 4 8 16]"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FULL = dict(num_channels=[128, 128, 128, 128], num_freqs=201, hidden=256, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3,
            dropout=0.0, sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--max-segments", type=int, nargs="*", default=[1, 4, 16])
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.general_beamformer import GeneralBeamformer
    spec = synth.gbf_param_spec(FULL["num_channels"], 201, 256, 3200, 2, 3, 3)
    m = GeneralBeamformer(**FULL).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()}, strict=True)
    m = m.cuda()
    L = int(args.seconds * 16000)
    print(f"GeneralBeamformer (config.yaml), {args.seconds:g} s per utterance, {torch.cuda.get_device_name(0)}, default max_segments {m.max_segments}")
    print(f"{'B':>4} {'path':>12} {'ms':>10} {'RTF':>8} {'peak MiB':>10}")
    for B in args.batches:
        mix = torch.from_numpy(synth.synth_utterances(B, L, 3, seed=1)[0]).cuda()
        rows = [("kernels", True)] + ([] if args.no_torch else [("restatement", False)])
        for name, hip in rows:
            m.use_hip_kernels(hip)
            with torch.no_grad():
                ms, mib = timed(lambda: m.realtime_process(mix), args.iters if hip else 1)
            print(f"{B:>4} {name:>12} {ms:>10.1f} {ms / 1000.0 / args.seconds:>8.4f} {mib:>10.0f}", flush=True)
        m.use_hip_kernels(True)
        default = m.max_segments
        for ns in args.max_segments:
            m.max_segments = ns
            with torch.no_grad():
                ms, mib = timed(lambda: m.realtime_process(mix), args.iters)
            print(f"{B:>4} {'max_seg=' + str(ns):>12} {ms:>10.1f} {ms / 1000.0 / args.seconds:>8.4f} {mib:>10.0f}", flush=True)
        m.max_segments = default
        K.PROF = {}
        with torch.no_grad():
            m.realtime_process(mix)
        prof = K.profile_summary()
        K.PROF = None
        tot = sum(v["ms"] for v in prof.values())
        print(f"     stages of one kernel-path call at B = {B} (event-bracketed launches, sum {tot:.1f} ms):")
        for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
            print(f"       {k:<18} {v['ms']:>9.2f} ms {v['launches']:>6} launches")


if __name__ == "__main__":
    main()
