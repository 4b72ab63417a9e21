"""CPU test of the fp16 pair's two stored weight planes (csrc/split_f16pair.h): tests/pair_w2_check.cpp, built with g++
in a temporary directory like f16_pair_check.cpp.  The kernels' two-plane instances fetch (w_lo, w_hi) and make 2^11 w_hi with one fp16
multiply; the check runs that multiply over every fp16 pattern below 2^4 (zeros and subnormals included) against plane 0 of
pair_weight_planes, and compares the two-plane matrix, W_hh, conv and skip images with planes 1 and 2 of the three-plane ones at the
indices the kernels read."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="g++ not available")
def test_two_stored_planes_scale_and_images(tmp_path):
    exe = str(tmp_path / "pair_w2_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "pair_w2_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
