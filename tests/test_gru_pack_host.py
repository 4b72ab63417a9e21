"""CPU test of the W_hh packing of the split-bf16 GRU step (csrc/gru_pack.h): tests/gru_pack_check.cpp, built with g++ in a
temporary directory, checks that the index map is a bijection, that every 64-lane x 16-byte fragment is contiguous and in the order
the kernel walks, and that the three bf16 planes sum back to every weight exactly."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

GXX = shutil.which("g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("gru_pack")
    exe = str(d / "gru_pack_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "gru_pack_check.cpp")], check=True)
    return exe


@pytest.mark.skipif(GXX is None, reason="g++ not available")
@pytest.mark.parametrize("hidden", [32, 64, 512])
def test_gru_pack_bijection_fragments_exact(checker, hidden):
    r = subprocess.run([checker, str(hidden)], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
