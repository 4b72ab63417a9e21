"""CPU-side checks of what the two inference engines share: the segment arithmetic the library computes (csrc/chain_plan.h, through
se_chunk_geometry) is engine.chain_geometry, and engine.SlotMap keeps the caller's rows.  No engine is constructed: se_create needs a
device."""
import ctypes as C

import numpy as np
import pytest

from speech_enhancement_mi_amd import engine


@pytest.mark.parametrize("K", [800, 3200])
def test_library_geometry_is_chain_geometry(K):
    """nseg, off0 and skip of se_chunk_geometry == engine.chain_geometry, exactly: both flags, every length in 1 .. 2K + 3 and the lengths of
    test_chain_cpu.py::test_ragged_geometry_is_segment_geometry_per_utterance."""
    lib = engine.load_library()
    rng = np.random.default_rng(0)
    lengths = list(range(1, 2 * K + 4)) + [1, 799, 1599, 1600, 1601, 3199, 3200, 3201, 4800, 4801, 16000, 59999] + \
        [int(v) for v in rng.integers(1, 60000, 40)]
    n, o, s = C.c_int64(), C.c_int64(), C.c_int64()
    for flag in (False, True):
        want = engine.chain_geometry(lengths, [flag] * len(lengths), K)
        got = []
        for L in lengths:
            assert lib.se_chunk_geometry(K, L, int(flag), C.byref(n), C.byref(o), C.byref(s)) == 0
            got.append((n.value, o.value, s.value))
        assert [g[0] for g in got] == want["Nb"]
        assert [g[1] for g in got] == want["off0"]
        assert [g[2] for g in got] == want["skip"]
    assert lib.se_chunk_geometry(K, 0, 0, C.byref(n), C.byref(o), C.byref(s)) != 0
    assert lib.se_chunk_geometry(0, 5, 0, C.byref(n), C.byref(o), C.byref(s)) != 0


def test_slot_map():
    m = engine.SlotMap()
    assert m.order is None and m.engine_index(2) == 2
    a = np.arange(15, dtype=np.float32)
    assert m.to_engine(a) is a and m.to_caller(a) is a            # the identity moves nothing
    assert m.choose([False] * 4, [8, 8, 6, 6]) is None            # already sorted
    assert m.choose([False] * 3, [5, 5, 5]) is None
    order = m.choose([False] * 4, [6, 8, 6, 8])                   # a fresh batch: most segments first, stable
    assert order == [1, 3, 0, 2]
    m.order = order
    assert m.choose([True, False, True, True], None) is order     # a carried batch keeps its map, whatever its lengths
    assert m.choose([True] * 3, None) is None                     # (a batch of another size has none)
    assert [m.order[m.engine_index(b)] for b in range(4)] == [0, 1, 2, 3]
    assert m.engine_index(7) == 7
    rng = np.random.default_rng(1)
    for shape, layered in (((2, 4, 3), True), ((4, 5), False)):
        a = rng.standard_normal(shape).astype(np.float32)
        e = m.to_engine(a.reshape(-1), layered, 2).reshape(shape)
        for s, b in enumerate(order):                             # engine row s = caller row order[s]
            assert np.array_equal(e[:, s] if layered else e[s], a[:, b] if layered else a[b])
        assert np.array_equal(m.to_caller(e.reshape(-1), layered, 2).reshape(shape), a)
        assert not np.array_equal(e, a)
