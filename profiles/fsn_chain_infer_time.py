"""Batched chunk-chain INFERENCE time of the FullSubNet engine: `--streams` ChunkChains (chunk lengths drawn as data_c.py draws them,
1 .. 3.75 s, own flag per chain) served through fsn_realtime_process_chains on FSN_FULL, timed with device events (median of `--iters`
after one warm-up call) against what a server had to do before the chains call existed:

  chains : FsnEngine.realtime_process_chains(x, flags, lengths): per-stream flags and step counters, every stream leaves its own state
  padded : FsnEngine.realtime_process(x, flag=False): every stream as long as the longest chunk of the step (wrong state for everyone
           who ends early; the only batched form of fsn_realtime_process), measured in step 0, or in every step with --padded-every-step

Step 0 of a set of chains is always a fresh batch (all flags 0), which the shim sorts by window count, so the engine launches every
window for the prefix of streams still running.  The later steps mix flags and keep the slots of step 0: every stream runs every window
(compaction of carried batches is out of scope), plus the save / restore traffic of the streams that end early.

    python profiles/fsn_chain_infer_time.py [--streams 256] [--steps 4] [--iters 3] [--precision 0] [--padded-only]

--padded-only runs the reference alone (it needs nothing but fsn_realtime_process, so it also runs on a checkout without the chains call)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.distill_train_time import ev_ms  # noqa: E402

FSN_FULL = dict(num_freqs=201, num_mics=3, fb_hidden=512, sb_hidden=384, num_layers=2, sb_neighbors=15, fb_neighbors=0, look_ahead=0,
                sample_rate=16000, segment_length=3200, win_length=25, hop_length=10, n_fft=400)  # config.yaml:153-172


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--precision", type=int, default=0)
    ap.add_argument("--padded-only", action="store_true")
    ap.add_argument("--padded-every-step", action="store_true")
    args = ap.parse_args()
    from speech_enhancement_mi_amd import engine, synth
    from speech_enhancement_mi_amd.datagen import ChunkChain
    c = FSN_FULL
    sd = synth.make_state_dict(synth.fsn_param_spec(c["num_freqs"], c["num_mics"], c["fb_hidden"], c["sb_hidden"], c["num_layers"],
                                                    c["sb_neighbors"], c["fb_neighbors"]), seed=0)

    def make_engine():
        e = engine.FsnEngine(precision=args.precision, **c)
        e.load_state_dict(sd)
        return e
    ec, er = make_engine(), make_engine()   # the chains keep their carried batch; the reference resets its own every call
    B = args.streams

    def utterances(seed):   # only lengths and flags matter here: 8 .. 15 s placeholders, cut by the chain
        rng = np.random.default_rng(seed)

        def make():
            L = int(rng.integers(8 * 16000, 15 * 16000))
            z = torch.zeros(1, L)
            return z, z, z, L
        return make
    chains = [ChunkChain(utterances(b), rng=np.random.default_rng(1000 + b)) for b in range(B)]
    print("| step | Lmax | mean / max length | flags set | windows (min / max) | streams ending early | chains ms | padded ms | chains / padded |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in range(args.steps):
        items = [next(ch) for ch in chains]
        lens, flags = [it["length"] for it in items], [bool(it["flag"]) for it in items]
        Lmax = max(lens)
        x = torch.randn(B, 3, Lmax, device="cuda") * 0.1
        out = torch.empty(B, Lmax, device="cuda")
        K, P = c["segment_length"], c["segment_length"] // 2   # the window arithmetic of fsn_realtime_process per stream
        nb = [2 * ((l + ld) + (K - (P + (l + ld) % K) % K) + P) // K for l, ld in ((l, 0 if f else P) for l, f in zip(lens, flags))]
        t_ch = t_pad = float("nan")
        if not args.padded_only:
            def run_chains():
                ec.realtime_process_chains(x, flags, lens, out=out)
            run_chains()   # warm-up (and the carried batch of the next step)
            torch.cuda.synchronize()
            t_ch = ev_ms(run_chains, args.iters)
        if s == 0 or args.padded_every_step:
            def run_padded():
                er.realtime_process(x, flag=False, out=out)
            run_padded()
            torch.cuda.synchronize()
            t_pad = ev_ms(run_padded, args.iters)
        print(f"| {s} | {Lmax} | {sum(lens) / len(lens) / Lmax:.2f} | {sum(flags)} / {B} | {min(nb)} / {max(nb)} | {sum(n < max(nb) for n in nb)} | "
              f"{t_ch:.1f} | {t_pad:.1f} | {t_ch / t_pad:.3f} |", flush=True)


if __name__ == "__main__":
    main()
