"""CPU tests of the fp16 pair format on the convolution / skip path (csrc/conv_weight_image.h, csrc/conv_p.hip.h).

1. tests/f16_pair_conv_check.cpp, built with g++ in a temporary directory like f16_pair_check.cpp: the k_conv_p and k_skip_p weight
   images hold (2^11 w_hi, w_lo, w_hi) at the indices the kernels read (one geometry per tap count 15, 9, 6 and 1, odd octet counts,
   the permuted epilogues); the skip output's bound on hand-made parameters (a row L1 norm that crosses 6e4 with every weight below
   16, one just below the limit); split2h(join2h(.)) is the identity on stored pairs.
2. The error model of test_f16_pair_cpu.py for a convolution-shaped contraction, K = taps x channels = 15 x 8, 9 x 64 and 1 x 32, in
   the kernels' term order (W0 x_hi, W1 x_hi, W2 x_lo into one sum, 2^-11 at the end): the pair against float64 stays in the 7-8e-8
   band that file reports.  A wrong term order or a missing scale leaves that band by an order of magnitude."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_f16_pair_cpu import _operand, _rel_rms, _sgemm, _split

GXX = shutil.which("g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("f16_pair_conv")
    exe = str(d / "f16_pair_conv_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "f16_pair_conv_check.cpp")], check=True)
    return exe


@pytest.mark.skipif(GXX is None, reason="g++ not available")
def test_weight_images_skip_bound_and_split_identity(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr


def _conv_pair(x, w):
    """k_conv_p<.., kF16Pair>: per K step W0 x_hi + W1 x_hi + W2 x_lo with W = (2^11 w_hi, w_lo, w_hi), one accumulator, 2^-11 last;
    exact products and float64 accumulation, so what is left is the error of the format"""
    xh, xl = _split(x, True)
    wh, wl = _split(w, True)
    w0 = (wh * 2048.0).astype(np.float16).astype(np.float64)
    assert np.all(np.isfinite(w0))
    return (w0 @ xh.T + wl @ xh.T + wh @ xl.T) / 2048.0


@pytest.mark.parametrize("taps,cin", [(15, 8), (9, 64), (1, 32)])
def test_conv_shaped_contraction_stays_in_the_pair_band(taps, cin):
    k = taps * cin
    rng = np.random.default_rng(2000 + k)
    for x_scale, w_scale in [(1e-3, 1e-3), (1e-3, 0.3), (1.0, 1e-2), (1.0, 0.3), (3e2, 1e-3), (3e2, 0.3)]:
        x, w = _operand(rng, 96, k, x_scale), _operand(rng, 64, k, w_scale)  # 96 positions x K patch, 64 output rows
        ref = w.astype(np.float64) @ x.astype(np.float64).T
        e_pair, e_f32 = _rel_rms(_conv_pair(x, w), ref), _rel_rms(_sgemm(w, x), ref)
        print(f"taps {taps} x Cin {cin} (K {k}) scales {x_scale:g} x {w_scale:g}: pair {e_pair:.2e}  fp32 {e_f32:.2e}")
        assert 6.0e-8 < e_pair < 9.0e-8, f"pair format error {e_pair:.3g} left the 7-8e-8 band: term order or scale"
        if k >= 120:  # (K = 32: the fp32 chain of 32 FMAs is itself near 1e-7)
            assert e_pair < e_f32
