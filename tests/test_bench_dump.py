"""bench.py --dump-outputs (CPU): the arrays land as DIR/<name>.npy in float32 / float64, at most 64 MB in all, and an output
over the budget is cut to the same seeded row sample on every run."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole(tmp_path):
    out = np.arange(12, dtype=np.float32).reshape(3, 4)
    loss = np.array([0.25], np.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"enhanced": out, "loss": loss, "ints": np.arange(5)})
    got = {f: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert sorted(got) == ["enhanced.npy", "ints.npy", "loss.npy"]
    np.testing.assert_array_equal(got["enhanced.npy"], out)
    assert got["loss.npy"].dtype == np.float64 and got["loss.npy"][0] == 0.25
    assert got["ints.npy"].dtype == np.float32


def test_large_outputs_are_sampled_within_budget_and_repeatably(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 16)
    big = np.random.default_rng(1).standard_normal((200, 256)).astype(np.float32)  # 200 KB > 64 KB
    flat = np.random.default_rng(2).standard_normal(50000)                          # float64, one long row
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"enhanced": big, "params": flat})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= (1 << 16) + 2 * 128  # + the .npy headers
    for name in ("enhanced", "params"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        np.testing.assert_array_equal(a, b)
    e = np.load(tmp_path / "a" / "enhanced.npy")
    assert e.shape[1] == 256 and 0 < e.shape[0] < 200
    assert all(any(np.array_equal(r, s) for s in big) for r in e)  # whole rows of the output, not a reshuffle
    assert np.load(tmp_path / "a" / "params.npy").dtype == np.float64
