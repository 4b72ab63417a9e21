"""bench.py --full (CPU): a plain run measures the headline figure alone - no profiled step, no secondary legs, no CPU
baselines - and --full brings all of them back.  The workload itself is stubbed; only the dispatch is under test."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def test_full_is_an_option_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse_args(["--full"]).full is True


@pytest.fixture
def stubbed(monkeypatch):
    calls = []

    def measure_crn(model, nfft, B, dtype, seconds, steps, warmup, rank, local_rank, world, backend, label_progress="", keep_output=False, profile=True):
        calls.append(("measure_crn", profile))
        info = dict(cfg=bench.crn_cfg(nfft, model), sd={}, variant=0, label="CRN", nseg=34, mflop_per_frame=1.0, dt=1.0, output=None)
        return 1000.0, 50.0, (dict(kernel="k") if profile else None), info

    monkeypatch.setattr(bench, "measure_crn", measure_crn)
    monkeypatch.setattr(bench, "secondary_lines", lambda *a: calls.append(("secondary",)) or [])
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a: calls.append(("cpu_baseline",)) or dict(value=1.0))
    monkeypatch.setattr(bench, "cpu_baseline_torch_guarded", lambda *a: calls.append(("cpu_baseline_torch",)) or [])
    return calls


def run_line(argv, capsys):
    bench.bench_crn(bench.parse_args(argv), 0, 0, 1, "none")
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_plain_run_measures_the_headline_only(stubbed, capsys):
    line = run_line(["--gpus", "1", "--steps", "3", "--warmup", "1"], capsys)
    assert stubbed == [("measure_crn", False)]
    assert (line["value"], line["ms_per_step"], line["unit"], line["higher_is_better"], line["dtype"]) == (1000.0, 50.0, "frames/s", True, "f32")
    assert line["metric"] == "streaming frames/sec @ b256 (CRN, 3200-samp 16 kHz)"
    assert line["roofline"] is None and line["cpu_baseline"] is None and "secondary" not in line


def test_full_run_adds_every_other_leg(stubbed, capsys):
    line = run_line(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"], capsys)
    assert stubbed == [("measure_crn", True), ("secondary",), ("cpu_baseline",), ("cpu_baseline_torch",)]
    assert line["roofline"] == dict(kernel="k") and line["secondary"] == [] and line["cpu_baseline"] == dict(value=1.0)
    assert (line["value"], line["ms_per_step"]) == (1000.0, 50.0)


def test_full_legs_can_still_be_skipped_one_by_one(stubbed, capsys):
    run_line(["--full", "--no-secondary", "--no-cpu-baseline"], capsys)
    assert stubbed == [("measure_crn", True)]
