"""DistillationCRN training micro-batch time: 8 utterances x 3 s, full-size variant-2 teacher (FULL400, frozen) and the 0.81 M-parameter
student, model(noisy, clean, length, flag=False) + backward (compute_loss + the feature loss), timed with device events after warm-up.
Split: teacher feature forward (no_grad), the distillation loss forward + backward on the same maps, and the rest (student forward +
backward, compute_loss).  The torch restatement on the same GPU for comparison.  For the loss kernels it also reports the bytes the
three passes move against the bytes of the maps they touch.

    python profiles/distill_train_time.py [--utts 8] [--seconds 3] [--iters 5] [--no-torch]"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FULL400 = dict(num_channels=[16, 32, 64, 128], num_freqs=201, hidden=512, segment_length=3200, num_layers=2, num_inputs=3, kernel_size=3,
               dropout=0.0, sample_rate=16000, win_length=25, hop_length=10, n_fft=400)


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
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.distillation_crn import DistillationCRN
    from speech_enhancement_mi_amd.training import TrainableStudentCRN
    c = FULL400
    spec = synth.crn_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["num_layers"], 3, 3, variant=2)
    t = TrainableStudentCRN(**c)
    t.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()})
    B, L = args.utts, int(args.seconds * 16000)
    mix, clean = synth.synth_utterances(B, L, 3, seed=11)
    x, cl = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
    lens = torch.full((B,), L, dtype=torch.int64, device="cuda")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "teacher.pth")
        torch.save(t.state_dict(), path)
        torch.manual_seed(0)
        base = DistillationCRN(**c, path=path)
    sd = base.state_dict()

    def measure(hip):
        m = DistillationCRN(**c)
        m.load_state_dict(sd)
        for p in m.teacher.parameters():
            p.requires_grad = False
        m = m.cuda().use_hip_kernels(hip)

        def step():
            loss = m(x, cl, lens, False)[0]
            loss.backward()
            m.zero_grad(set_to_none=True)

        def teacher():
            with torch.no_grad():
                m.teacher.realtime_process_train(x, False, features=True)
        with torch.no_grad():
            _, ft = m.teacher.realtime_process_train(x, False, features=True)
            _, fs = m.student.realtime_process_train(x, False, features=True)
        fs = [f.detach().requires_grad_(True) for f in fs]

        def dloss():
            m.distillation_loss(ft, fs).backward()
        step(), teacher(), dloss()  # warm-up: library load, workspaces
        torch.cuda.synchronize()
        total, tt, tl = ev_ms(step, args.iters), ev_ms(teacher, args.iters), ev_ms(dloss, args.iters)
        return total, tt, tl, ft, fs

    rows = [("hip", True)] + ([] if args.no_torch else [("torch", False)])
    for name, hip in rows:
        total, tt, tl, ft, fs = measure(hip)
        print(f"{name:5s}: {total:8.1f} ms per micro-batch ({B} x {args.seconds:g} s) = teacher features {tt:.1f} + distillation loss fwd+bwd "
              f"{tl:.1f} + student fwd+bwd and compute_loss {total - tt - tl:.1f}")
        if hip:
            S = ft[0].shape[0]
            touched = sum(4 * (a.numel() + b.numel()) for a, b in zip(ft, fs))
            ws = sum(4 * S * a.shape[1] * b.shape[1] for a, b in zip(ft, fs))  # dW row partials (written + folded)
            moved = 3 * touched + sum(4 * b.numel() for b in fs) + 2 * ws
            print(f"       loss kernels: maps touched {touched / 1e6:.1f} MB, moved by the three passes {moved / 1e6:.1f} MB "
                  f"({moved / touched:.2f}x); {moved / tl / 1e9:.2f} TB/s effective at {tl:.2f} ms")


if __name__ == "__main__":
    main()
