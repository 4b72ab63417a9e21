"""losses.pesq_loss / GTSA.compute_loss on the CPU: the torch restatement `_pesq_d` against tests/golden/pesq_golden.npz, which
tests/golden/make_golden_pesq.py wrote from the GENUINE reference code (utility.pesq_loss, GTSA.compute_loss; torchaudio's Spectrogram
restated there -> parity unpinned at that boundary).

THE BAR.  The fixture holds, per case, the reference's float32 value and gradient and the same from `_pesq_d` in float64, and `e_ref`:
the float32 reference's own distance from float64 - absolute for the value, relative L2 (per row, on the stored every-5th samples) for
the gradient - the largest over the cases (4.7e-7 and 1.08e-5).  The restatement in float32 sums in another order than the reference
(notably in the FFT) and that is all it may differ by: it gets 4 x e_ref against float64, hence 5 x e_ref against the reference itself.
The maker asserted that float64 stays 1e-5 away from every branch of the loss on every case, so none of this measures a flipped branch."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_gtsa as mgt  # noqa: E402
import make_golden_pesq as mkp  # noqa: E402
from loss_inputs import make_loss_inputs  # noqa: E402

from speech_enhancement_mi_amd import losses  # noqa: E402
from speech_enhancement_mi_amd.gtsa import GTSA  # noqa: E402

CASES = ("row0", "row1", "row2", "row3", "e4864", "e5120", "e7424", "e7680", "zero", "asym")


@pytest.fixture(scope="module")
def pg():
    return np.load(os.path.join(ROOT, "tests", "golden", "pesq_golden.npz"))


@pytest.fixture(scope="module")
def cases():
    return mkp.cases()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run_alone(c, p, dtype=torch.float32):
    pt = torch.from_numpy(p).to(dtype).requires_grad_(True)
    v = losses._pesq_d(torch.from_numpy(c).to(dtype), pt, torch.tensor([c.shape[1]]))
    v.sum().backward()
    return float(v.detach()[0]), pt.grad[0].numpy()


@pytest.fixture(scope="module")
def alone32(cases):
    """`_pesq_d` in float32, every case at B = 1: computed once, shared"""
    return {k: run_alone(*cases[k]) for k in CASES}


def test_fixture_condition(pg):
    assert list(pg["case_names"]) == list(CASES)
    assert float(pg["margins"].min()) >= 1e-5, dict(zip(pg["margin_names"], pg["margins"]))
    assert 0 < pg["e_ref"][0] < 1e-5 and 0 < pg["e_ref"][1] < 1e-3
    assert np.abs(pg["row0_val"][0] - -0.2301) < 1e-4 and np.abs(pg["row3_val"][0] - -0.6817) < 1e-4


@pytest.mark.parametrize("name", CASES)
def test_restatement_float32_vs_fixture(name, pg, alone32):
    v, g = alone32[name]
    ev, eg = pg["e_ref"]
    dv, dg = abs(v - float(pg[f"{name}_val64"][0])), rel_l2(g[::5], pg[f"{name}_grad64_s5"])
    print(f"{name}: value {v:+.7f} |d64| {dv:.2e} (bar {4 * ev:.2e}); gradient rel L2 vs float64 {dg:.2e} (bar {4 * eg:.2e})")
    assert np.isfinite(g).all()
    assert dv <= 4 * ev and dg <= 4 * eg
    assert abs(v - float(pg[f"{name}_val"][0])) <= 5 * ev + 6e-8 * abs(v)  # + the float32 the reference's value is stored in
    assert rel_l2(g[::5], pg[f"{name}_grad_s5"]) <= 5 * eg
    assert abs(np.linalg.norm(g) / float(pg[f"{name}_grad_norm"][0]) - 1) <= 5 * eg


def test_float64_is_the_fixtures_truth(pg, cases):
    """the float64 columns of the fixture are this code: re-derived to rounding on the T = 31 case"""
    v, g = run_alone(*cases["e7680"], dtype=torch.float64)
    assert abs(v - float(pg["e7680_val64"][0])) < 1e-12
    assert rel_l2(g[::5], pg["e7680_grad64_s5"]) < 1e-10


def test_zero_stretch_has_zero_gradient(alone32):
    """frames of zero disturbance (clean and prediction zeroed on [5000, 8000)): the frames wholly inside, centred on 5376 .. 7680, get none"""
    g = alone32["zero"][1]
    assert np.isfinite(g).all() and np.all(g[5376:7681] == 0) and np.abs(g[:5000]).max() > 0


def ragged_batch():
    clean, pred, lens = make_loss_inputs()
    for b in range(4):
        clean[b, lens[b]:] = np.nan
        pred[b, lens[b]:] = np.nan
    return clean, pred, lens


def test_ragged_batch_equals_rows_alone_and_permutes(pg):
    clean, pred, lens = ragged_batch()
    ev, eg = pg["e_ref"]

    def run(order):
        p = torch.from_numpy(pred[order]).requires_grad_(True)
        v = losses.pesq_loss(torch.from_numpy(clean[order]), p, torch.from_numpy(lens[order]), reduction="batch")
        v.sum().backward()
        return v.detach().numpy(), p.grad.numpy()

    v, g = run([0, 1, 2, 3])
    for b in range(4):
        assert abs(v[b] - float(pg[f"row{b}_val64"][0])) <= 4 * ev
        assert rel_l2(g[b, :lens[b]:5], pg[f"row{b}_grad64_s5"]) <= 4 * eg
        assert np.all(g[b, lens[b]:] == 0)  # nothing at or beyond lens[b] is read
    perm = [2, 0, 3, 1]
    vp, gp = run(perm)
    for i, b in enumerate(perm):
        assert abs(vp[i] - v[b]) <= 4 * ev and rel_l2(gp[i, :lens[b]], g[b, :lens[b]]) <= 4 * eg
    # "mean" is the batch mean
    m = losses.pesq_loss(torch.from_numpy(clean), torch.from_numpy(pred), torch.from_numpy(lens))
    assert m.dim() == 0 and abs(float(m) - v.mean()) <= 4 * ev
    full = losses.pesq_loss(torch.from_numpy(clean[:1]), torch.from_numpy(pred[:1]), None, reduction="batch")  # lens=None: the full rows
    assert abs(float(full[0]) - v[0]) <= 4 * ev


def test_refuses_fewer_than_20_frames():
    x = torch.zeros(2, 4863)
    with pytest.raises(NotImplementedError, match="pesq_loss has no value for fewer than 20 spectrogram frames"):
        losses.pesq_loss(x, x, None)
    y = torch.zeros(2, 6000)
    for lens in ([6000, 4863], np.array([4863, 6000]), torch.tensor([6000, 100])):
        with pytest.raises(NotImplementedError, match="pesq_loss has no value for fewer than 20 spectrogram frames"):
            losses.pesq_loss(y, y, lens)
    assert losses.pesq_loss(y + 0.01, y + 0.02, [6000, 4864], reduction="batch").shape == (2,)


def test_short_row_inside_the_restatement_is_nan_with_zero_gradient(cases):
    """`_pesq_d` itself (what a device-resident lens reaches): NaN for the short row, zero gradient, the other row untouched"""
    c, p = cases["e7680"]
    c2, p2 = np.concatenate([c, c]), np.concatenate([p, p])
    pt = torch.from_numpy(p2).requires_grad_(True)
    v = losses._pesq_d(torch.from_numpy(c2), pt, torch.tensor([4000, 7680]))
    v[1].backward()
    assert torch.isnan(v[0]) and torch.isfinite(v[1])
    assert torch.all(pt.grad[0] == 0) and torch.isfinite(pt.grad[1]).all() and pt.grad[1].abs().max() > 0


def test_gtsa_compute_loss_vs_reference(pg, cases):
    """the triple of the reference's GTSA.compute_loss on row 1.  mae: 5 x e_ref as above.  sisnr = -20 log10 of a ratio of float32 norms
    over 20000 samples, each good to about 1e-6 relative: 20 / ln 10 x 2e-6 = 2e-5 absolute."""
    c, p = cases["row1"]
    ev, eg = pg["e_ref"]
    pt = torch.from_numpy(p).requires_grad_(True)
    loss, mae, sisnr = GTSA(**mgt.TINY).compute_loss(torch.from_numpy(c), pt, torch.tensor([c.shape[1]]))
    loss.backward()
    want = pg["gtsa_loss"]
    assert abs(float(mae.detach()) - want[1]) <= 5 * ev + 6e-8 and abs(float(sisnr.detach()) - want[2]) <= 2e-5
    assert abs(float(loss.detach()) - want[0]) <= 0.7 * 5 * ev + 0.3 * 2e-5 + 2.4e-7  # + half an ulp of the float32 sum at 3.4
    assert rel_l2(pt.grad[0].numpy()[::5], pg["gtsa_grad_s5"]) <= 5 * eg


def test_gtsa_compute_loss_nan_rule(cases):
    c, p = cases["e5120"]
    p = p.copy()
    p[0, 1000] = np.nan
    out = GTSA(**mgt.TINY).compute_loss(torch.from_numpy(c), torch.from_numpy(p), torch.tensor([5120]))
    assert all(float(o) == 0.0 for o in out)


def test_gradient_against_central_differences(cases):
    """float64 on the T = 21 slice: the autograd gradient along 4 random directions against central differences of the value.  A step
    of 1e-6 of the signal's RMS per sample keeps every comparison on its side (the fixture's margins are 1e-5 and more); the
    difference quotient's own error is about eps_machine |f| / (step |g.d|) ~ 1e-9 relative plus O(step^2), so 1e-6 is a wide berth for
    rounding and a narrow one for a wrong or missing term (the smallest term of the backward, the level path, carries 1e-3 of it)."""
    c, p = cases["e5120"]
    ct, p0 = torch.from_numpy(c).double(), torch.from_numpy(p).double()
    ln = torch.tensor([5120])
    pt = p0.clone().requires_grad_(True)
    losses._pesq_d(ct, pt, ln).sum().backward()
    rms = float(p0.pow(2).mean().sqrt())
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        d = torch.randn(p0.shape, generator=gen, dtype=torch.float64) * rms
        h = 1e-6
        fd = float(losses._pesq_d(ct, p0 + h * d, ln)[0] - losses._pesq_d(ct, p0 - h * d, ln)[0]) / (2 * h)
        an = float((pt.grad * d).sum())
        print(f"directional derivative: autograd {an:+.9e} central difference {fd:+.9e}")
        assert abs(fd - an) <= 1e-6 * abs(an)
