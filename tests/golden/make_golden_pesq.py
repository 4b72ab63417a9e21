#!/usr/bin/env python3
"""PESQ-loss fixture (tests/golden/pesq_golden.npz) from the GENUINE reference code, run on the CPU (needs the reference checkout):

    python tests/golden/make_golden_pesq.py

`utility.pesq_loss` (utility.py:615-814) and `GTSA.compute_loss` (GTSA.py:411-433) run from the reference's source files unmodified,
behind make_golden.py's import placeholders.  pesq_loss calls torchaudio.transforms.Spectrogram(1024, 512, 256, power=2), which is
absent from the reference tree and from this image: the stand-in below restates it over torch.stft (periodic Hann(win_length) centred
in n_fft, centre reflect padding, |X|^power), the same stand-in make_golden_loss.py uses => PARITY UNPINNED AT THE TORCHAUDIO BOUNDARY.
Only DATA is written; no reference source text is copied.

Inputs: loss_inputs.make_loss_inputs(), every row cut to its own length and run at B = 1 (the reference has no value at B > 1: it reuses
the name `h` across its loop over the batch).  Cases, by name:
  row0 .. row3   the four rows at their own lengths (24000, 20000, 16001, 24000)
  e4864, e5120, e7424, e7680   row 0 cut to T = 20, 21, 30, 31 frames: one syllable block with the shortest tail; the first two-block lengths
  zero           row 2 cut to 12000 samples with clean AND prediction zeroed on [5000, 8000): frames of zero disturbance
  asym           the first 8000 samples of row 1 against 0.3 x clean + an amplitude-modulated 5 kHz tone: the only case whose asymmetric
                 disturbance is not zero (the factor ratio ** 1.2 stays below 3 on speech-like predictions); largest per-frame value 7.8
Per case: `<c>_val` the reference's value, `<c>_grad_s5` every 5th sample of d loss / d pred, `<c>_grad_norm`; `<c>_val64`,
`<c>_grad64_s5`, `<c>_grad64_norm` the same from losses._pesq_d in float64 on the same inputs; `<c>_e_ref` = [|val - val64|,
||grad_s5 - grad64_s5|| / ||grad64_s5||], the float32 reference's own distance from float64.  `e_ref` = the largest of each over the
cases: the restatement and the kernels each get 4 x e_ref against float64 (they sum in another order, notably in the FFT).
`gtsa_loss` = the three outputs of the reference's GTSA.compute_loss on row 1, `gtsa_grad_s5` its gradient.

CONDITION: the float64 restatement must stay 1e-5 (relative) away from every branch of the loss on every case - band thresholds, the
1e7 silence level, the equalisation and recurrence clamps, the dead zone +-m, the asymmetry's 3 and 12 (where the disturbance is not
zero), the cap at 45 - so that float32 and float64 take the same branches and e_ref measures rounding only.  Asserted here; the smallest
margin per family goes into the fixture (`margin_names`, `margins`).  A case that violates it gets another gain in GAIN below, never a
looser check."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shared import placeholders)
import make_golden_gtsa as mgt  # noqa: E402

EDGES = (4864, 5120, 7424, 7680)
ZERO = (2, 12000, 5000, 8000)  # row, length, zeroed [from, to)
GAIN = {}  # case name -> gain on the prediction, should a case sit on a branch (none does)
MARGIN = 1e-5


def cases():
    """name -> (clean [1, L], pred [1, L]) float32 numpy"""
    from loss_inputs import make_loss_inputs
    clean, pred, lens = make_loss_inputs()
    out = {}
    for b in range(4):
        out[f"row{b}"] = (clean[b:b + 1, :lens[b]].copy(), pred[b:b + 1, :lens[b]].copy())
    for n in EDGES:
        out[f"e{n}"] = (clean[:1, :n].copy(), pred[:1, :n].copy())
    b, n, z0, z1 = ZERO
    c, p = clean[b:b + 1, :n].copy(), pred[b:b + 1, :n].copy()
    c[:, z0:z1] = 0.0
    p[:, z0:z1] = 0.0
    out["zero"] = (c, p)
    t = np.arange(8000) / 16000.0
    tone = 0.25 * np.sin(2 * np.pi * 5000 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))
    out["asym"] = (clean[1:2, :8000].copy(), (0.3 * clean[1:2, :8000] + tone[None]).astype(np.float32))
    for k, g in GAIN.items():
        out[k] = (out[k][0], (out[k][1] * np.float32(g)).astype(np.float32))
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mg._install_import_placeholders()
    import torchaudio
    import torchaudio.transforms as TT

    class Spectrogram(torch.nn.Module):  # torchaudio.transforms.Spectrogram(n_fft, win_length, hop_length, power)(waveform[time]) -> [freq, time']
        def __init__(self, n_fft=400, win_length=None, hop_length=None, power=2.0):
            super().__init__()
            self.n_fft, self.win, self.hop, self.power = n_fft, win_length or n_fft, hop_length or (win_length or n_fft) // 2, power
            self.window = torch.hann_window(self.win)

        def forward(self, x):
            s = torch.stft(x, self.n_fft, self.hop, self.win, self.window.to(x.device), center=True, pad_mode="reflect",
                           normalized=False, onesided=True, return_complex=True)
            return (s.real ** 2 + s.imag ** 2).pow(0.5 * self.power)

    TT.Spectrogram = Spectrogram
    torchaudio.transforms = TT
    import GTSA
    import utility
    from speech_enhancement_mi_amd import losses

    out, margins, e_val, e_grad = {}, {}, [], []
    for name, (c, p) in cases().items():
        L = c.shape[1]
        ct, pt = torch.from_numpy(c), torch.from_numpy(p).requires_grad_(True)
        v = utility.pesq_loss(ct, pt, torch.tensor([L]))
        v.backward()
        p64 = torch.from_numpy(p).double().requires_grad_(True)
        mg_case = {}
        v64 = losses._pesq_d(ct.double(), p64, torch.tensor([L]), margins=mg_case)[0]
        v64.backward()
        g, g64 = pt.grad[0].double()[::5], p64.grad[0][::5]
        assert torch.isfinite(pt.grad).all() and torch.isfinite(p64.grad).all(), name
        v, v64 = v.detach(), v64.detach()
        ev, eg = abs(float(v) - float(v64)), float((g - g64).norm() / g64.norm())
        out[f"{name}_val"] = np.array([float(v)], np.float32)
        out[f"{name}_grad_s5"] = mg.t2n(pt.grad[0])[::5]
        out[f"{name}_grad_norm"] = np.array([float(pt.grad.norm())], np.float32)
        out[f"{name}_val64"] = np.array([float(v64)], np.float64)
        out[f"{name}_grad64_s5"] = g64.numpy().copy()
        out[f"{name}_grad64_norm"] = np.array([float(p64.grad.norm())], np.float64)
        out[f"{name}_e_ref"] = np.array([ev, eg], np.float64)
        e_val.append(ev)
        e_grad.append(eg)
        print(f"{name:6s} L {L:6d}  ref {float(v):+.6f}  f64 {float(v64):+.9f}  e_ref value {ev:.2e} grad {eg:.2e}  |grad| {float(pt.grad.norm()):.3e}  "
              f"smallest margin {min(mg_case.values()):.2e} ({min(mg_case, key=mg_case.get)})")
        bad = {k: m for k, m in mg_case.items() if m < MARGIN}
        assert not bad, f"case {name} sits on a branch: {bad}; give it another gain in GAIN"
        for k, m in mg_case.items():
            margins[k] = min(margins.get(k, float("inf")), m)
    out["e_ref"] = np.array([max(e_val), max(e_grad)], np.float64)
    out["margin_names"] = np.array(sorted(margins))
    out["margins"] = np.array([margins[k] for k in sorted(margins)], np.float64)
    out["case_names"] = np.array(list(cases()))

    # ---- GTSA.compute_loss on row 1 -------------------------------------------------------------------------------------------
    c, p = cases()["row1"]
    model = GTSA.GTSA(**mgt.TINY)
    pt = torch.from_numpy(p).requires_grad_(True)
    loss, mae, sisnr = model.compute_loss(torch.from_numpy(c), pt, torch.tensor([c.shape[1]]))
    loss.backward()
    out["gtsa_loss"] = np.array([float(loss), float(mae), float(sisnr)], np.float32)
    out["gtsa_grad_s5"] = mg.t2n(pt.grad[0])[::5]
    path = os.path.join(HERE, "pesq_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote pesq_golden.npz", os.path.getsize(path), "bytes; e_ref", out["e_ref"], "margins", dict(zip(out["margin_names"], out["margins"])))
    print("GTSA.compute_loss", out["gtsa_loss"])


if __name__ == "__main__":
    main()
