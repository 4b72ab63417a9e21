"""Batched chunk-chain INFERENCE time: `--streams` ChunkChains (chunk lengths drawn as data_c.py draws them, 1 .. 3.75 s, own flag per
chain) served through se_realtime_process_chains on the FULL400 CRN, timed with device events after warm-up against the uniform batch:

  chains : Engine.realtime_process_chains(x, flags, lengths): per-stream flags, every stream leaves its own continuation state
  uniform: Engine.realtime_process(x, flag=False): every stream as long as the longest chunk of the step

(A ragged call, Engine.realtime_process(x, flag, lengths=lengths) / se_realtime_process_ragged, is the chains route with one flag for
every stream; the separate `ragged` leg recorded in DESIGN.md 6 predates that.)
Step 0 of a set of chains is always a fresh batch (all flags 0), which the shim sorts by segment count; the later steps mix flags and
keep the slots of step 0, so they are compacted only as far as their segment counts happen to be sorted.

    python profiles/chain_infer_time.py [--streams 256] [--steps 4] [--iters 3] [--precision 0]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from profiles.distill_train_time import FULL400, ev_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--precision", type=int, default=0)
    args = ap.parse_args()
    from speech_enhancement_mi_amd import engine, synth
    from speech_enhancement_mi_amd.datagen import ChunkChain
    c = FULL400
    spec = synth.crn_param_spec(c["num_channels"], c["num_freqs"], c["hidden"], c["num_layers"], 3, 3)
    sd = synth.make_state_dict(spec, seed=0)

    def make_engine():
        e = engine.Engine(engine.make_config(c["num_channels"], c["num_freqs"], c["hidden"], c["segment_length"], c["num_layers"], c["num_inputs"],
                                             c["kernel_size"], c["sample_rate"], c["win_length"], c["hop_length"], c["n_fft"], precision=args.precision), 0)
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
    tot = dict(chains=0.0, uniform=0.0)
    print("| step | Lmax | mean / max length | flags set | segments (min / max) | streams ending early | chains ms | uniform ms | chains / uniform |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in range(args.steps):
        items = [next(ch) for ch in chains]
        lens, flags = [it["length"] for it in items], [bool(it["flag"]) for it in items]
        Lmax = max(lens)
        x = torch.randn(B, 3, Lmax, device="cuda") * 0.1
        out = torch.empty(B, Lmax, device="cuda")
        nb = engine.chain_geometry(lens, flags, c["segment_length"])["Nb"]

        def run_chains():
            ec.realtime_process_chains(x, flags, lens, out=out)

        def run_uniform():
            er.realtime_process(x, flag=False, out=out)
        run_chains(), run_uniform()   # warm-up (and the carried batch of the chains)
        torch.cuda.synchronize()
        t = dict(chains=ev_ms(run_chains, args.iters), uniform=ev_ms(run_uniform, args.iters))
        for k in tot:
            tot[k] += t[k]
        print(f"| {s} | {Lmax} | {sum(lens) / len(lens) / Lmax:.2f} | {sum(flags)} / {B} | {min(nb)} / {max(nb)} | {sum(n < max(nb) for n in nb)} | "
              f"{t['chains']:.1f} | {t['uniform']:.1f} | {t['chains'] / t['uniform']:.3f} |")
    n = args.steps
    print(f"{B} streams, {n} steps, precision {args.precision}: chains {tot['chains'] / n:.1f} ms, uniform at Lmax "
          f"{tot['uniform'] / n:.1f} ms per call; chains / uniform {tot['chains'] / tot['uniform']:.3f}")


if __name__ == "__main__":
    main()
