"""CPU tests of the fp16 pair operand format (csrc/split_f16pair.h).

1. A numpy model of the format: operands split as the kernels split them, exact products, float64 accumulation - what is left is
   the error of the FORMAT (the representation of both operands and the dropped lo * lo term).  It must stay below the error of a plain
   fp32 GEMM of the same operands (fp32 FMA accumulation along K, the arithmetic of the fp32 MFMA chain), for the K of the bottleneck
   GEMMs and activation scales 1e-3 .. 3e2; the same split WITHOUT the 2^11 scale on the low part must not - which is why the scale
   exists.  Weight scales stop at 0.3 (elements up to 50 x the scale, and the engine's range guard keeps |w| < 2^4).
2. tests/f16_pair_check.cpp, built with g++ in a temporary directory like gru_pack_check.cpp: split2h round trips, clamping, and the
   weight packers' planes (2^11 hi, lo, hi) at the indices the kernels read."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GXX = shutil.which("g++")
SCALE = np.float32(2048.0)


def _operand(rng, rows, k, scale):
    """elements spread log-uniformly over 1e-4 x .. 50 x the scale, random signs"""
    mag = np.exp(rng.uniform(np.log(1e-4), np.log(50.0), size=(rows, k)))
    return (scale * mag * rng.choice([-1.0, 1.0], size=(rows, k))).astype(np.float32)


def _split(x, scaled):
    x = np.clip(x, -65504.0, 65504.0).astype(np.float32)
    hi = x.astype(np.float16)
    r = x - hi.astype(np.float32)  # exact in fp32
    lo = (r * SCALE if scaled else r).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _pair_gemm(a, w, scaled):
    """three terms, smallest first, in float64: a_hi W1 + a_lo W2 + a_hi W0 with W = (2^11 hi, lo, hi) (scaled) or (hi, lo, hi)"""
    ah, al = _split(a, scaled)
    wh, wl = _split(w, scaled)
    if scaled:
        w0 = (wh * 2048.0).astype(np.float16).astype(np.float64)  # exact; finite below 2^4
        assert np.all(np.isfinite(w0))
        return (ah @ wl.T + al @ wh.T + ah @ w0.T) / 2048.0
    return ah @ wl.T + al @ wh.T + ah @ wh.T


def _sgemm(a, w):
    """fp32 GEMM: one fp32 FMA per k, in K order"""
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a64[:, k:k + 1] * w64[None, :, k]).astype(np.float32)
    return acc.astype(np.float64)


def _rel_rms(x, ref):
    return float(np.sqrt(np.mean((x - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


@pytest.mark.parametrize("k", [512, 576, 1920])
def test_pair_gemm_error_below_fp32_gemm_and_unscaled_is_not(k):
    rng = np.random.default_rng(1000 + k)
    unscaled_worse = 0
    for a_scale, w_scale in [(1e-3, 1e-3), (1e-3, 0.3), (1.0, 1e-2), (1.0, 0.3), (3e2, 1e-3), (3e2, 0.3)]:
        a, w = _operand(rng, 48, k, a_scale), _operand(rng, 40, k, w_scale)
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        e_pair, e_raw, e_f32 = _rel_rms(_pair_gemm(a, w, True), ref), _rel_rms(_pair_gemm(a, w, False), ref), _rel_rms(_sgemm(a, w), ref)
        print(f"K {k} scales {a_scale:g} x {w_scale:g}: pair {e_pair:.2e}  unscaled {e_raw:.2e}  fp32 gemm {e_f32:.2e}")
        assert e_pair < e_f32, f"pair format error {e_pair:.3g} is not below the fp32 GEMM's {e_f32:.3g}"
        unscaled_worse += e_raw > e_f32
        if a_scale == 1e-3 and w_scale == 1e-3:  # the low parts of both operands sit in fp16 subnormals
            assert e_raw > e_f32 and e_raw > 10 * e_pair, f"unscaled split unexpectedly accurate: {e_raw:.3g}"
    assert unscaled_worse >= 1


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("f16_pair")
    exe = str(d / "f16_pair_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "f16_pair_check.cpp")], check=True)
    return exe


@pytest.mark.skipif(GXX is None, reason="g++ not available")
@pytest.mark.parametrize("hidden", [32, 64])
def test_split2h_round_trip_clamp_and_weight_planes(checker, hidden):
    r = subprocess.run([checker, str(hidden)], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
