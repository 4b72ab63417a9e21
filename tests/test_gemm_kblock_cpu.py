"""CPU test of the K-blocked pair operands of k_gemm_p (csrc/gemm_kblock.h): tests/gemm_kblock_check.cpp, built with g++ in a
temporary directory like pair_w2_check.cpp.  The K-blocked weight image against planes (w_lo, w_hi) of pair_weight_matrix2 at every index
the kernel stages and reads (K = 32, 512, 2176; N with and without a 128-column tail), the LDS swizzle as a bijection per 1-KB run, and a
brute-force bank model of the ds_read_b128 lane groups (no conflict for both K steps, lane halves and planes)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="g++ not available")
def test_kblocked_images_swizzle_and_banks(tmp_path):
    exe = str(tmp_path / "gemm_kblock_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "gemm_kblock_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
