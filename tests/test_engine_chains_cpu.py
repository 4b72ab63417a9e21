"""CPU-side checks of se_realtime_process_chains: the shim's per-stream geometry is the training side's, and the new entry point is part
of the C ABI (declared, exported, listed) at an unchanged ABI version."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT


def test_chain_geometry_is_ragged_geometry():
    """engine.chain_geometry (what se_realtime_process_chains computes per stream on the host) == train_stages.ragged_geometry for the
    length and flag lists of test_chain_cpu.py::test_ragged_geometry_is_segment_geometry_per_utterance."""
    from speech_enhancement_mi_amd.engine import chain_geometry
    from speech_enhancement_mi_amd.train_stages import ragged_geometry
    rng = np.random.default_rng(0)
    lengths = [1, 799, 1599, 1600, 1601, 3199, 3200, 3201, 4800, 4801, 16000, 59999] + [int(v) for v in rng.integers(1, 60000, 40)]
    flags = [bool(v) for v in rng.integers(0, 2, len(lengths))]
    for Ks, hop, n_fft in ((3200, 160, 400), (3200, 160, 512), (1600, 160, 400)):
        q, g = ragged_geometry(lengths, flags, Ks, hop, n_fft, [5, 16, 32]), chain_geometry(lengths, flags, Ks)
        for key in ("Nb", "off0", "skip", "N"):
            assert g[key] == q[key], key
        # a reset stream starts one segment length before its first sample, a continuing one half a segment
        assert all(o == (-Ks // 2 if f else -Ks) for o, f in zip(g["off0"], flags))


def test_flags_convention():
    """One value (a bool, the reference trainer's one-element flag tensor) stays a scalar flag; one value per stream is a chains call."""
    import pytest
    import torch
    from speech_enhancement_mi_amd.engine import _flags_of
    assert _flags_of(True, 3) is True and _flags_of(0, 3) is False and _flags_of(torch.tensor([True]), 3) is True
    assert _flags_of(torch.tensor([True, False, True]), 3) == [True, False, True] and _flags_of([0, 1], 2) == [False, True]
    with pytest.raises(RuntimeError, match="flags for a batch"):
        _flags_of([True, False], 3)


def test_chains_entry_point_declared_exported_and_listed():
    from speech_enhancement_mi_amd import engine
    text = open(os.path.join(ROOT, "include", "se_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+se_realtime_process_chains\s*\(([^)]*)\)\s*;", code)
    assert m, "se_realtime_process_chains is not declared in se_engine.h outside comments"
    args = m.group(1)
    assert "const int64_t *lengths_host" in args and "const uint8_t *flags_host" in args and "int64_t max_length" in args
    assert re.search(r"\bint\s+se_chunk_geometry\s*\(", code), "se_chunk_geometry is not declared in se_engine.h outside comments"
    lib = ctypes.CDLL(engine.LIB_PATH)
    for name in ("se_realtime_process_chains", "se_chunk_geometry"):
        assert name in engine.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.se_abi_version() == 5
