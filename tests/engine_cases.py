"""What the GPU tests of the inference engines share (as chain_cases.py does for the chunk chains): the names of every environment knob
the library reads, one builder of an engine under a pinned environment, the two small geometries and the two-call snapshot."""
import os

import numpy as np
import torch

from conftest import FULL512, fsn_spec, spec_of_variant
from speech_enhancement_mi_amd import synth

# Every name the C sources hand to getenv (tests/test_route_knobs_cpu.py keeps the list equal to them).  The two names ending in the
# prefix of a plan or decoder level are completed at run time: SE_CONVP_NT_<plan>, SE_DEC_PAIR_dec<j>.
ROUTE_KNOBS = frozenset((
    "SE_CONVP_NT", "SE_CONVP_NT_", "SE_CONVP_VERBOSE", "SE_DBG_SKIP", "SE_DEC_PAIR", "SE_DEC_PAIR_dec", "SE_F16_PAIR", "SE_F16_PAIR_CONV",
    "SE_FSN_BIG", "SE_FSN_PIPELINE", "SE_GEMM_KBLOCK", "SE_GEMM_P", "SE_GEMM_SKINNY_ROWS", "SE_GRU_DIRECT", "SE_GRU_SPLIT", "SE_IO_FUSE",
    "SE_PAIR_W3", "SE_PIPELINE", "SE_PRE_P", "SE_RAGGED_COMPACT", "SE_SKIP_DEPTH", "SE_SKIP_MIN_BATCH"))
_PREFIXES = ("SE_CONVP_NT_", "SE_DEC_PAIR_dec")

# The plane GEMM route's smallest 512-point shape (K = 544 = 17 chunks); a single octet on levels 1 and 2: the skip gate reads the clamped
# odd octet.
SMALL = dict(FULL512, num_channels=[8, 8, 16, 32], hidden=64)
# Some waves of the skip gate own no tile: a segment has at least 17 frames (the largest dilation history), so fewer than 8 tiles of 32
# positions need at most 13 bins on the deepest skip level.  128-point FFT at 4 kHz (25 ms window = 100 samples, 17 frames): 65 bins,
# 33 / 17 / 9 on levels 1 to 3, 17 x 9 = 153 positions = 5 tiles for the 8 waves of a workgroup.
SHORT = dict(SMALL, sample_rate=4000, n_fft=128, num_freqs=65, segment_length=640)


def pin_env(monkeypatch, env=None):
    """Unset every knob the library reads, then set `env`: the knobs are read when an engine is created."""
    for k in list(os.environ):
        if k in ROUTE_KNOBS or k.startswith(_PREFIXES):
            monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def make_engine(cfg, monkeypatch=None, env=None, *, variant=0, precision=0, seed=0, sd=None, device=0):
    """An Engine of the geometry `cfg` with `sd`, or the hash weights of `seed`, loaded.  With a monkeypatch it is created under `env`
    and no other knob (pin_env); without one the environment is the caller's."""
    from speech_enhancement_mi_amd import engine
    if monkeypatch is not None:
        pin_env(monkeypatch, env)
    c = engine.make_config(cfg["num_channels"], cfg["num_freqs"], cfg["hidden"], cfg["segment_length"], cfg["num_layers"],
                           cfg["num_inputs"], cfg["kernel_size"], cfg["sample_rate"], cfg["win_length"], cfg["hop_length"], cfg["n_fft"],
                           variant=variant, precision=precision)
    e = engine.Engine(c, device)
    e.load_state_dict(sd if sd is not None else synth.make_state_dict(spec_of_variant(cfg, variant), seed=seed))
    return e


def make_fsn_engine(cfg, *, precision=0, seed=0, sd=None, device=0):
    from speech_enhancement_mi_amd import engine
    e = engine.FsnEngine(cfg["num_freqs"], cfg["num_mics"], cfg["fb_model_hidden_size"], cfg["sb_model_hidden_size"], cfg["num_layers"],
                         cfg["sb_num_neighbors"], cfg["fb_num_neighbors"], cfg["look_ahead"], cfg["sample_rate"], cfg["segment_length"],
                         cfg["win_length"], cfg["hop_length"], cfg["n_fft"], device=device, precision=precision)
    e.load_state_dict(sd if sd is not None else synth.make_state_dict(fsn_spec(cfg), seed=seed))
    return e


def cuda(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # (torch wants a writable array; shared inputs are read-only)


def utterances(batch, length, seed, mics=3):
    """A read-only [batch, mics, length] mixture to share among the tests of a module."""
    mix, _ = synth.synth_utterances(batch, length, mics, seed=seed)
    mix.setflags(write=False)
    return mix


def carried_state(e, cfg):
    """The GRU state h and the conv time buffers buf<i>, by name."""
    return {k: np.array(e.export_state(k), copy=True) for k in ["h"] + [f"buf{i}" for i in range(len(cfg["num_channels"]))]}


def snapshot(e, cfg, y, taps):
    """What one call left behind, by name: the output y, the taps and the carried state - in that order."""
    return {"out": y, **{t: np.array(e.read_tap(t), copy=True) for t in taps}, **carried_state(e, cfg)}


def two_call_snapshots(e, cfg, x, lengths, taps):
    """x[:, :, :l1] with flag=False, then the next l2 samples with the carried state (lengths = (l1, l2)): the snapshot after each call"""
    l1, l2 = lengths
    return [snapshot(e, cfg, e.realtime_process(cuda(x[:, :, lo:hi]), flag=flag).cpu().numpy(), taps)
            for lo, hi, flag in ((0, l1, False), (l1, l1 + l2, True))]
