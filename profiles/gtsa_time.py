"""GTSA inference time (hash weights): realtime_process of B utterances x 3 s, flag=False, under no_grad, in both fixture geometries
(tiny: 2 layers, fn_dim 32, maxlen 50; full: 6 layers, fn_dim 1024, maxlen 210).  For each batch size: the kernel path and the torch
restatement on the same GPU (median ms over --iters after one warm-up, real-time factor = seconds per second of audio of one
utterance, peak torch.cuda.max_memory_allocated), then a per-stage breakdown of one kernel-path call through train_ops.PROF with the
share of the attention launches.

    python profiles/gtsa_time.py [--batches 1 8 64] [--seconds 3] [--iters 3] [--geometries tiny full] [--no-torch]"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TINY = dict(num_mics=3, num_freqs=201, segment_length=3200, num_layers=2, num_heads=5, model_dim=201, fn_dim=32, maxlen=50, dropout=0.0,
            sample_rate=16000, win_length=25, hop_length=10, n_fft=400)
GEOMS = dict(tiny=TINY, full=dict(TINY, num_layers=6, fn_dim=1024, maxlen=210))


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
    ap.add_argument("--geometries", nargs="+", default=["tiny", "full"])
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.gtsa import GTSA
    L = int(args.seconds * 16000)
    for tag in args.geometries:
        cfg = GEOMS[tag]
        spec = synth.gtsa_param_spec(cfg["num_mics"], cfg["num_freqs"], cfg["num_layers"], cfg["fn_dim"], cfg["maxlen"])
        m = GTSA(**cfg).eval()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.gtsa_state_dict(spec, seed=0).items()}, strict=True)
        m = m.cuda()
        print(f"GTSA {tag} ({cfg['num_layers']} layers, fn_dim {cfg['fn_dim']}, maxlen {cfg['maxlen']}), {args.seconds:g} s per utterance, "
              f"{torch.cuda.get_device_name(0)}, max_segments {m.max_segments}")
        print(f"{'B':>4} {'path':>12} {'ms':>10} {'RTF':>8} {'peak MiB':>10}")
        for B in args.batches:
            mix = torch.from_numpy(synth.synth_utterances(B, L, 3, seed=1)[0]).cuda()
            for name, hip in [("kernels", True)] + ([] if args.no_torch else [("restatement", False)]):
                m.use_hip_kernels(hip)
                with torch.no_grad():
                    ms, mib = timed(lambda: m.realtime_process(mix), args.iters)
                print(f"{B:>4} {name:>12} {ms:>10.1f} {ms / 1000.0 / args.seconds:>8.4f} {mib:>10.0f}", flush=True)
            m.use_hip_kernels(True)
            K.PROF = {}
            with torch.no_grad():
                m.realtime_process(mix)
            prof = K.profile_summary()
            K.PROF = None
            tot = sum(v["ms"] for v in prof.values())
            attn = prof.get("k_gtsa_attn", dict(ms=0.0))["ms"]
            print(f"     stages of one kernel-path call at B = {B} (event-bracketed launches, sum {tot:.1f} ms; attention {100 * attn / max(tot, 1e-9):.1f} %):")
            for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
                print(f"       {k:<18} {v['ms']:>9.2f} ms {v['launches']:>6} launches", flush=True)


if __name__ == "__main__":
    main()
