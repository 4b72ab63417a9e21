"""CPU test of the fixed-geometry Stockham passes (csrc/fft_lds.h: fft_fixed_pass): tests/fft_fixed_check.cpp, built with g++ in a
temporary directory, runs them and the run-time passes (fft_pass) on the same frames, thread by thread as the STFT kernels do.  The
two must give the same bits, and rfft_post of the result must be the real FFT of the frame."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GXX = shutil.which("g++")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("fft_fixed")
    exe = str(d / "fft_fixed_check")
    subprocess.run([GXX, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "fft_fixed_check.cpp")], check=True)
    return exe


def _frames(n_fft, nfft, seed):
    """Seeded frames of the size of the quantity test_stft_istft bounds with 3e-5: noise of rms 0.25 under the engine's window
    (hamming(400) centred in n_fft), |X| up to about 10 (the golden STFT reaches 13.5).  Frame 1 is silent."""
    rng = np.random.default_rng(seed)
    w = np.zeros(n_fft)
    left = (n_fft - 400) // 2
    w[left:left + 400] = 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(400) / 400)
    x = (0.25 * rng.standard_normal((nfft, n_fft)) * w).astype(np.float32)
    x[1] = 0.0
    return x


# (frames, threads): the kernels' own 7 frames on 448 threads (one butterfly per thread and pass at 512), a partial last round,
# and fewer threads than butterflies so that every thread makes several trips
@pytest.mark.skipif(GXX is None, reason="g++ not available")
@pytest.mark.parametrize("n_fft", [400, 512])
@pytest.mark.parametrize("nfft,nth", [(7, 448), (3, 448), (7, 64), (5, 100)])
def test_fixed_passes_equal_generic_and_rfft(checker, tmp_path, n_fft, nfft, nth):
    x = _frames(n_fft, nfft, seed=n_fft + nfft)
    fin, fout = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    x.tofile(fin)
    r = subprocess.run([checker, str(n_fft), str(nfft), str(nth), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # non-zero: the two forms of the passes differ in some bit (or the plan order does)
    X = np.fromfile(fout, np.float32).reshape(nfft, n_fft // 2 + 1, 2)
    ref = np.fft.rfft(x.astype(np.float64), axis=-1)
    err = max(np.abs(X[..., 0] - ref.real).max(), np.abs(X[..., 1] - ref.imag).max())
    print(f"n_fft {n_fft} frames {nfft} threads {nth}: max abs err vs numpy.fft.rfft {err:.3e}, max |X| {np.abs(ref).max():.2f}")
    assert err < 3e-5
    assert np.all(X[1] == 0.0)  # a silent frame gives exact zeros
