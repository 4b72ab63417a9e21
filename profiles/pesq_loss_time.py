"""pesq_loss time, forward + backward: the se_loss_pesq_* kernels (csrc/se_pesq.hip) against the torch restatement losses._pesq_d on the
same GPU, for B utterances x 3 s of synthetic speech and a degraded copy (median ms over --iters after one warm-up, event-timed).

Every (B, path) step runs in a fresh child process under its own time limit (--limit seconds); the first step that fails or runs
out of time ends the script, nothing more is started on the GPU after it.

    python profiles/pesq_loss_time.py [--batches 1 8 64] [--seconds 3] [--iters 20] [--limit 120]"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(B, seconds, path, iters):
    import torch
    from speech_enhancement_mi_amd import losses, synth
    L = int(seconds * 16000)
    mix, clean = synth.synth_utterances(B, L, 3, seed=1)
    noise = synth.hash_tensor("pesq.time", (B, L)) * 0.05
    c = torch.from_numpy(clean.astype("float32")).cuda()
    p = torch.from_numpy((0.8 * clean + 0.3 * (mix[:, 0] - clean) + noise).astype("float32")).cuda().requires_grad_(True)
    losses.PESQ_KERNELS = path == "kernels"

    def run():
        p.grad = None
        losses.pesq_loss(c, p, None).backward()

    run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    print(f"{B:>4} {path:>12} {ts[len(ts) // 2]:>10.2f} {ts[0]:>10.2f}   value {float(losses.pesq_loss(c, p.detach(), None)):+.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--step", nargs=2, metavar=("B", "PATH"), help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        step(int(args.step[0]), args.seconds, args.step[1], args.iters)
        return 0
    print(f"pesq_loss forward + backward, {args.seconds:g} s per utterance")
    print(f"{'B':>4} {'path':>12} {'median ms':>10} {'min ms':>10}", flush=True)
    for B in args.batches:
        for path in ("kernels", "restatement"):
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--seconds", str(args.seconds), "--iters", str(args.iters), "--step", str(B), path],
                                    timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step B = {B} {path} ended with status {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
