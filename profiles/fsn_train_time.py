"""FullSubNet training micro-batch time: 8 utterances x 3 s, full compute_loss, forward + backward of
TrainableFullSubNet.use_hip_kernels(True), timed with device events after warm-up; the torch fp32 restatement on the same GPU for
comparison.  Prints ms, utterances/s and the algorithmic FLOPs of the LSTM / linear contractions from the shapes.

    python profiles/fsn_train_time.py [--utts 8] [--seconds 3] [--iters 5] [--no-torch] [--adam]

Kernel split: run it under `rocprofv3 --kernel-trace --stats -- python profiles/fsn_train_time.py --no-torch`."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FSN_FULL = dict(num_freqs=201, look_ahead=0, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15, fb_output_activate_function="ReLU",
                sb_output_activate_function=False, fb_model_hidden_size=512, sb_model_hidden_size=384, num_mics=3, norm_type="offline_laplace_norm",
                num_groups_in_drop_band=2, num_layers=2, weight_init=False, sample_rate=16000, segment_length=3200, win_length=25, hop_length=10,
                n_fft=400)


def flops(B, N, T=21, F=201, M=3, Hf=512, Hs=384, SI=32):
    """forward / backward matrix FLOPs of the two LSTMs + their output layers (2 x MACs)."""
    fb_rows, sb_rows = N * B * T, N * B * F * T
    fwd = 2 * fb_rows * (4 * Hf * (F * M + Hf) + 4 * Hf * (2 * Hf) + F * Hf) + 2 * sb_rows * (4 * Hs * (SI + Hs) + 4 * Hs * (2 * Hs) + 2 * Hs)
    # backward: recurrent dh (K = 4H) per layer, dx of layer 1, weight gradients of both matrices per layer, output layers
    bptt = 2 * fb_rows * 2 * 4 * Hf * Hf + 2 * sb_rows * 2 * 4 * Hs * Hs
    dx = 2 * fb_rows * (4 * Hf * Hf + F * Hf) + 2 * sb_rows * (4 * Hs * Hs + 4 * Hs)
    wgrad = 2 * fb_rows * (4 * Hf * (F * M + Hf) + 4 * Hf * 2 * Hf + F * Hf) + 2 * sb_rows * (4 * Hs * (SI + Hs) + 4 * Hs * 2 * Hs + 2 * Hs)
    return fwd, bptt, dx, wgrad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--adam", action="store_true", help="also an Adam step per iteration: the next forward then re-uploads the changed "
                    "weights to the engine (host copy + split planes) and the backward rebuilds its transposed fp32 weights")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    spec = synth.fsn_param_spec(201, 3, 512, 384, 2, 15, 0)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec, seed=0).items()}
    B, L = args.utts, int(args.seconds * 16000)
    mix, clean = synth.synth_utterances(B, L, 3, seed=11)
    x = torch.from_numpy(mix).cuda()
    src = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    lens = torch.full((B,), L, dtype=torch.int64, device="cuda")

    def timed(hip, iters):
        m = TrainableFullSubNet(**FSN_FULL)
        m.load_state_dict(sd)
        m = m.cuda().use_hip_kernels(hip)
        opt = torch.optim.Adam(m.parameters(), lr=3e-4) if args.adam else None

        def step():
            pred, crm, s, xf = m.realtime_process(x, src, False, train=False)
            loss = m.compute_loss(src[:, 0], pred, xf, s, crm, lens)[0]
            loss.backward()
            if opt is not None:
                opt.step()
            m.zero_grad(set_to_none=True)
        step()  # warm-up: library load, workspace allocation
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        del m
        torch.cuda.empty_cache()
        return float(np.median(ts)), float(np.min(ts))

    P = 1600
    Lp = L + P
    gap = 3200 - (P + Lp % 3200) % 3200
    N = 2 * (Lp + gap + P) // 3200
    fwd, bptt, dx, wg = flops(B, N)
    tot = fwd + bptt + dx + wg
    med, best = timed(True, args.iters)
    print(f"HIP   {B} x {args.seconds:g} s (N = {N} windows){' + Adam step' if args.adam else ''}: median {med:.1f} ms, best {best:.1f} ms, {B / med * 1e3:.1f} utt/s, "
          f"{tot / med / 1e9:.1f} TFLOP/s algorithmic")
    print(f"FLOPs: forward {fwd / 1e12:.2f} T, BPTT {bptt / 1e12:.2f} T, dx {dx / 1e12:.2f} T, weight gradients {wg / 1e12:.2f} T, "
          f"total {tot / 1e12:.2f} T (>= {tot / 157e12 * 1e3:.0f} ms at the 157 TF fp32-MFMA peak)")
    if not args.no_torch:
        med_t, best_t = timed(False, max(1, args.iters // 2))
        print(f"torch fp32 restatement: median {med_t:.1f} ms, best {best_t:.1f} ms, {B / med_t * 1e3:.1f} utt/s")


if __name__ == "__main__":
    main()
