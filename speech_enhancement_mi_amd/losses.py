"""Training loss of the reference contract, device-resident: compute_loss = 0.7 * stoi_loss + 0.3 * (-SI-SNR)
(reference CRN.py:593-617).

* `cal_si_snr` restates utility.py:207-223.  On GPU tensors it runs as ONE fused HIP kernel pair (csrc/se_loss.hip through the
  C ABI `se_loss_sisnr_fwd/bwd`): per-utterance moment reductions in the forward, a closed-form elementwise backward - no
  Python loop over the batch, no host hop.  On CPU tensors (unit tests, CPU training) the same formula runs in torch.
* `stoi_loss` on CUDA tensors runs on the `se_loss_stoi_*` kernels (csrc/se_stoi.hip: 7 launches forward, 4 backward; `_StoiHip`).
  `_stoi_d` restates utility.py:821-916 (+ thirdoct 480-518, removeSilentFrames 521-571) as batched, differentiable torch
  tensor code that stays on the tensors' device: the CPU path and the checker the kernels are tested against (STOI_KERNELS = False).  The reference moves every utterance to the CPU and loops in Python
  (`y_pred_batch.cpu()`, utility.py:845-880); here the whole batch is processed at once with validity masks - the
  data-dependent lengths (silent-frame removal) never come back to the host, so there is no synchronisation in the loss.
  The two torchaudio==0.7.2 transforms it calls are absent from the reference tree and this image and are restated:
  Resample(16000, 10000) = Kaldi LinearResample (the reference's in-tree copy of the algorithm is augment.py:234-545) as a
  5-phase strided convolution; Spectrogram(512, 256, 128, power=2) over torch.fft.  PARITY UNPINNED AT THE TORCHAUDIO
  BOUNDARY; pinned above it by tests/golden/loss_golden.npz (the reference's own stoi_loss / compute_loss code run on these
  restated transforms, values AND the gradient w.r.t. the prediction).
* `pesq_loss` (utility.py:615-814) and `gtsa_compute_loss` = GTSA.compute_loss (GTSA.py:411-433: 0.7 * pesq_loss + 0.3 * (-SI-SNR)).  On
  CUDA tensors the `se_loss_pesq_*` kernels (csrc/se_pesq.hip: 2 launches forward, 3 backward; `_PesqHip`); `_pesq_d` restates the
  reference's per-utterance CPU code with its Python loop over frames as batched, differentiable torch code in float32 or float64: the
  CPU path and the checker (PESQ_KERNELS = False).  torchaudio's Spectrogram(1024, 512, 256, power=2) is restated over torch.fft:
  PARITY UNPINNED AT THE TORCHAUDIO BOUNDARY, pinned above it by tests/golden/pesq_golden.npz.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as Fn

SMALL = float(np.finfo("float").eps)  # utility.py:478 `smallVal`


# =====================================================================================================================
# SI-SNR (utility.py:207-223)
# =====================================================================================================================
def _cal_si_snr_torch(separated, source, length=None, eps=1e-8):
    B = len(separated)
    total = 0.0
    for i in range(B):
        n = separated.shape[-1] if length is None else int(length[i])
        s, r = separated[i, :n], source[i, :n]
        s = s - torch.mean(s, dim=-1, keepdim=True)
        r = r - torch.mean(r, dim=-1, keepdim=True)
        true = torch.sum(s * r, dim=-1, keepdim=True) * r / (torch.norm(r, dim=-1, keepdim=True) ** 2 + eps)
        total = total + 20 * torch.log10(eps + torch.norm(true, dim=-1) / (torch.norm(s - true, dim=-1) + eps))
    return total / B


class _SiSnrHip(torch.autograd.Function):
    """mean over the batch of the per-utterance SI-SNR, forward and backward on hand-written HIP kernels."""

    @staticmethod
    def forward(ctx, separated, source, lens_dev):
        from . import engine
        lib = engine.load_library()
        sep = separated.contiguous().float()
        src = source.contiguous().float()
        B, L = sep.shape
        per = torch.empty(B, dtype=torch.float32, device=sep.device)
        stats = torch.empty(B * 8, dtype=torch.float64, device=sep.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.se_loss_sisnr_fwd(C.c_void_p(sep.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(lens_dev.data_ptr()), B, L,
                                   C.c_void_p(per.data_ptr()), C.c_void_p(stats.data_ptr()), st)
        if rc != 0:
            raise RuntimeError(f"se_loss_sisnr_fwd failed ({rc})")
        ctx.save_for_backward(sep, src, lens_dev, stats)
        return per.mean()

    @staticmethod
    def backward(ctx, g):
        from . import engine
        lib = engine.load_library()
        sep, src, lens_dev, stats = ctx.saved_tensors
        B, L = sep.shape
        grad = torch.empty_like(sep)
        gscale = (g.float() / B).reshape(1).contiguous()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.se_loss_sisnr_bwd(C.c_void_p(sep.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(lens_dev.data_ptr()), B, L,
                                   C.c_void_p(stats.data_ptr()), C.c_void_p(gscale.data_ptr()), C.c_void_p(grad.data_ptr()), st)
        if rc != 0:
            raise RuntimeError(f"se_loss_sisnr_bwd failed ({rc})")
        return grad, None, None


def _lens_tensor(length, B, L, device):
    if length is None:
        return torch.full((B,), L, dtype=torch.int64, device=device)
    t = torch.as_tensor(length).to(device=device, dtype=torch.int64)
    return torch.clamp(t, 0, L)


def cal_si_snr(separated, source, length=None, eps=1e-8):
    """utility.cal_si_snr: mean over the batch of 20 log10(eps + |s_target| / (|s - s_target| + eps)) on the first length[i]
    samples, means removed."""
    if separated.is_cuda and separated.dim() == 2:
        return _SiSnrHip.apply(separated, source, _lens_tensor(length, separated.shape[0], separated.shape[1], separated.device))
    return _cal_si_snr_torch(separated, source, length, eps)


# =====================================================================================================================
# STOI loss (utility.py:821-916)
# =====================================================================================================================
def _resample_plan(orig_freq=16000, new_freq=10000, lowpass_filter_width=6):
    """Kaldi LinearResample polyphase filter (augment.py:478-545), float32 arithmetic like the reference's torch code."""
    base = math.gcd(orig_freq, new_freq)
    stride, phases = orig_freq // base, new_freq // base
    f32 = np.float32
    cutoff = 0.99 * 0.5 * min(orig_freq, new_freq)
    width = lowpass_filter_width / (2.0 * cutoff)
    out_t = np.arange(0.0, phases, dtype=f32) / f32(new_freq)
    lo = np.ceil((out_t - f32(width)) * f32(orig_freq))
    hi = np.floor((out_t + f32(width)) * f32(orig_freq))
    W = int((hi - lo + 1).max())
    idx = lo[:, None] + np.arange(W, dtype=f32)[None, :]
    dt = (idx / f32(orig_freq)) - out_t[:, None]
    w = np.zeros_like(dt)
    inside = np.abs(dt) < f32(width)
    w[inside] = (0.5 * (1 + np.cos(f32(2 * math.pi * cutoff / lowpass_filter_width) * dt[inside]))).astype(f32)
    nz = dt != 0.0
    w[nz] *= (np.sin(f32(2 * math.pi * cutoff) * dt[nz]) / (f32(math.pi) * dt[nz])).astype(f32)
    w[~nz] *= f32(2 * cutoff)
    w /= f32(orig_freq)
    return lo.astype(np.int64), w.astype(f32), stride, phases


_PLAN = {}


def _plan(device):
    key = str(device)
    if key not in _PLAN:
        first, w, stride, phases = _resample_plan()
        n = np.arange(256)
        # thirdoct(fs=10000, nfft=512, num_bands=15, min_freq=150) (utility.py:480-518)
        f = np.linspace(0, 10000, 513, dtype=np.float32)[:257]
        k = np.arange(15, dtype=np.float64)
        lo_f, hi_f = 150 * np.power(2.0, (2 * k - 1) / 6), 150 * np.power(2.0, (2 * k + 1) / 6)
        obm = np.zeros((15, 257), np.float32)
        for i in range(15):
            obm[i, int(np.argmin(np.square(f - np.float32(lo_f[i])))):int(np.argmin(np.square(f - np.float32(hi_f[i]))))] = 1
        win512 = np.zeros(512, np.float32)
        win512[128:384] = (0.5 - 0.5 * np.cos(2 * np.pi * n / 256)).astype(np.float32)  # periodic Hann(256) centred in 512
        lo_bin = [int(np.argmin(np.square(f - np.float32(lo_f[i])))) for i in range(15)]
        hi_bin = [int(np.argmin(np.square(f - np.float32(hi_f[i])))) for i in range(15)]
        _PLAN[key] = dict(first=[int(v) for v in first], w=torch.from_numpy(w).to(device), stride=stride, phases=phases,
                          hann_sym=torch.from_numpy(np.hanning(256).astype(np.float32)).to(device),  # np.hanning(256), utility.py:522
                          win512=torch.from_numpy(win512).to(device), obm=torch.from_numpy(obm).to(device),
                          # tables of the kernel form (csrc/se_stoi.hip)
                          first_dev=torch.tensor([int(v) for v in first], dtype=torch.int32, device=device),
                          hann_per=torch.from_numpy(win512[128:384].copy()).to(device),
                          band_lo=torch.tensor(lo_bin, dtype=torch.int32, device=device), band_hi=torch.tensor(hi_bin, dtype=torch.int32, device=device))
    return _PLAN[key]


def _resample_batch(x, lens, P):
    """x [B, L] (only the first lens[i] samples of row i count) -> y [B, Lo] at 10 kHz and the per-row output counts."""
    B, L = x.shape
    x = x * (torch.arange(L, device=x.device)[None, :] < lens[:, None])
    stride, phases, W = P["stride"], P["phases"], P["w"].shape[1]
    # LinearResample::GetNumOutputSamples with ticks of 1/80000 s: 5 ticks per input, 8 per output sample
    interval = lens * 5
    last = torch.div(interval, 8, rounding_mode="floor")
    n_out = torch.where(interval > 0, torch.where(last * 8 == interval, last, last + 1), torch.zeros_like(last))
    Lo = (L * 5 + 7) // 8
    padl = max(0, -min(P["first"]))
    K = (Lo + phases - 1) // phases
    padr = stride * K + W + max(P["first"]) + 8
    xp = Fn.pad(x, (padl, padr))[:, None, :]
    y = x.new_zeros(B, K * phases)
    # One banded contraction per phase, written as strided views + a matrix-vector product instead of Fn.conv1d: MIOpen's
    # strided 1-D convolution on a sliced input view read past the end of its allocation (GPU memory access fault in the
    # forward or backward of this loss, depending on where the caching allocator had placed the tensor).
    for i in range(phases):
        start = padl + P["first"][i]
        frames = xp[:, 0, start:].unfold(1, W, stride)[:, :K]  # [B, K, W] view: frames[b, k, j] = xp[b, start + k stride + j]
        y[:, i::phases] = torch.matmul(frames.double(), P["w"][i].double()).to(y.dtype)  # (STOI's silent-frame selection is sensitive to the last bits)
    y = y[:, :Lo]
    return y * (torch.arange(Lo, device=x.device)[None, :] < n_out[:, None]), n_out


def _stoi_d(y_true, y_pred, lens):
    """D[i] of utility.py:856-911 for the whole batch, on the inputs' device; differentiable w.r.t. y_pred."""
    dev = y_pred.device
    P = _plan(dev)
    B = y_pred.shape[0]
    t10, n10 = _resample_batch(y_true.float(), lens, P)
    p10, _ = _resample_batch(y_pred.float(), lens, P)
    # ---- removeSilentFrames (utility.py:521-571): 256-sample frames every 128 samples, energy from the CLEAN signal ----
    n1 = torch.div(n10, 256, rounding_mode="floor")
    n2 = torch.div(n10 - 128, 256, rounding_mode="floor")
    nf = torch.clamp(n1 + n2, min=0)
    Lo = t10.shape[1]
    if Lo < 256:
        return torch.full((B,), 0.99, device=dev)
    ft, fp = t10.unfold(1, 256, 128), p10.unfold(1, 256, 128)  # [B, Fu, 256]
    Fu = ft.shape[1]
    valid = torch.arange(Fu, device=dev)[None, :] < nf[:, None]
    w = P["hann_sym"]
    energy = 20 * torch.log10(torch.sqrt(((w ** 2)[None, None, :] * ft.detach() ** 2).sum(-1)) / 16.0 + SMALL)
    emax = torch.where(valid, energy, torch.full_like(energy, -float("inf"))).max(dim=1, keepdim=True).values
    keep = valid & ((energy - emax + 40) > 0)
    nk = keep.sum(1)
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)  # kept frames first, in time order
    kept = (torch.arange(Fu, device=dev)[None, :] < nk[:, None])[..., None]
    gt = torch.gather(ft * w, 1, order[..., None].expand(-1, -1, 256)) * kept
    gp = torch.gather(fp * w, 1, order[..., None].expand(-1, -1, 256)) * kept

    def ola(v):  # [first half of frame 0 | frame k first half + frame k-1 second half | second half of the last]
        return (Fn.pad(v[..., :128], (0, 0, 0, 1)) + Fn.pad(v[..., 128:], (0, 0, 1, 0))).reshape(B, -1)

    st, sp = ola(gt), ola(gp)
    Ls = 128 * (nk + 1)  # samples after silence removal
    # ---- Spectrogram(512, 256, 128, power=2): centre reflect padding at each row's OWN end ----
    n = torch.arange(st.shape[1] + 512, device=dev)[None, :] - 256
    m = n.abs()
    m = torch.where(m >= Ls[:, None], 2 * (Ls[:, None] - 1) - m, m).clamp(0, st.shape[1] - 1)
    T = nk + 2  # 1 + Ls // 128 frames
    Tm = Fu + 2
    tvalid = torch.arange(Tm, device=dev)[None, :] < T[:, None]

    def oct_env(s):
        fr = torch.gather(s, 1, m).unfold(1, 512, 128)[:, :Tm] * P["win512"]
        S = torch.fft.rfft(fr, dim=-1)
        pw = S.real ** 2 + S.imag ** 2  # [B, Tm, 257]
        return torch.sqrt(pw @ P["obm"].T + 1e-14) * tvalid[..., None]  # [B, Tm, 15]

    Ot, Op = oct_env(st), oct_env(sp)
    c = 5.62341325
    if Tm >= 30:  # 30-frame envelope vectors (utility.py:887-892)
        X = Ot.unfold(1, 30, 1).double()  # [B, Mm, 15, 30]
        Y = Op.unfold(1, 30, 1).double()
        Mi = T - 29
        mvalid = (torch.arange(X.shape[1], device=dev)[None, :] < Mi[:, None])[..., None]
        alpha = X.norm(dim=-1, keepdim=True) / (Y.norm(dim=-1, keepdim=True) + SMALL)
        yc = torch.minimum(Y * alpha, X + X * c)
        xn = X - X.mean(-1, keepdim=True)
        xn = xn / (xn.norm(dim=-1, keepdim=True) + SMALL)
        yn = yc - yc.mean(-1, keepdim=True)
        yn = yn / (yn.norm(dim=-1, keepdim=True) + SMALL)
        d_full = ((xn * yn).sum(-1) * mvalid).sum((1, 2)) / (15.0 * Mi.clamp(min=1))
    else:
        d_full = torch.zeros(B, dtype=torch.float64, device=dev)
    # fewer than 30 frames: ONE vector per band spanning all T frames (utility.py:882-885)
    Tc = min(Tm, 29)
    Xs, Ys = Ot[:, :Tc].transpose(1, 2).double(), Op[:, :Tc].transpose(1, 2).double()  # [B, 15, Tc], zero beyond T
    cnt = T.clamp(min=1, max=Tc).double()[:, None, None]
    sv = tvalid[:, None, :Tc]
    alpha = Xs.norm(dim=-1, keepdim=True) / (Ys.norm(dim=-1, keepdim=True) + SMALL)
    yc = torch.minimum(Ys * alpha, Xs + Xs * c)
    xn = (Xs - Xs.sum(-1, keepdim=True) / cnt) * sv
    xn = xn / (xn.norm(dim=-1, keepdim=True) + SMALL)
    yn = (yc - yc.sum(-1, keepdim=True) / cnt) * sv
    yn = yn / (yn.norm(dim=-1, keepdim=True) + SMALL)
    d_few = (xn * yn).sum((1, 2)) / 15.0
    d = torch.where(T >= 30, d_full, d_few).float()
    return torch.where(Ls <= 512, torch.full_like(d, 0.99), d)


STOI_KERNELS = True  # CUDA tensors: csrc/se_stoi.hip (6 + 4 launches); False: the batched torch restatement _stoi_d (~150 ops), the checker


class _StoiHip(torch.autograd.Function):
    """D[i] of utility.py:856-911 on the se_loss_stoi_* kernels; gradient to the prediction only."""

    @staticmethod
    def forward(ctx, y_true, y_pred, lens):
        from . import engine as _engine
        lib = _engine.load_library()
        P = _plan(y_pred.device)
        B, L = y_pred.shape
        yt, yp, ln = y_true.detach().contiguous().float(), y_pred.detach().contiguous().float(), lens.contiguous().to(torch.int64)
        ws = torch.empty(int(lib.se_loss_stoi_ws_floats(B, L)), dtype=torch.float32, device=y_pred.device)
        D = torch.empty(B, dtype=torch.float32, device=y_pred.device)
        st = C.c_void_p(torch.cuda.current_stream(y_pred.device).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        tabs = (p(P["w"]), p(P["first_dev"]), int(P["w"].shape[1]), p(P["hann_sym"]), p(P["hann_per"]), p(P["band_lo"]), p(P["band_hi"]))
        if lib.se_loss_stoi_fwd(p(yt), p(yp), p(ln), B, L, *tabs, p(ws), p(D), st):
            raise RuntimeError(lib.se_loss_stoi_last_error().decode())
        ctx.save_for_backward(ln, ws)
        ctx.shape = (B, L)
        ctx.dev = y_pred.device
        return D

    @staticmethod
    def backward(ctx, gD):
        from . import engine as _engine
        lib = _engine.load_library()
        ln, ws = ctx.saved_tensors
        B, L = ctx.shape
        P = _plan(ctx.dev)
        g = gD.contiguous().float()
        dpred = torch.empty(B, L, dtype=torch.float32, device=ctx.dev)
        st = C.c_void_p(torch.cuda.current_stream(ctx.dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        tabs = (p(P["w"]), p(P["first_dev"]), int(P["w"].shape[1]), p(P["hann_sym"]), p(P["hann_per"]), p(P["band_lo"]), p(P["band_hi"]))
        if lib.se_loss_stoi_bwd(p(g), p(ln), B, L, *tabs, p(ws), p(dpred), st):
            raise RuntimeError(lib.se_loss_stoi_last_error().decode())
        return None, dpred, None


def _stoi_ws_views(ws, B, L):
    """Named views into the kernels' workspace (the layout of csrc/se_stoi.hip:stoi_shape) - for tests and debugging."""
    Lo = (L * 5 + 7) // 8
    Fu = (Lo - 256) // 128 + 1
    Tm = Fu + 2
    off = [0]

    def take(n):
        at = off[0]
        off[0] += (n + 3) & ~3
        return at
    o = {k: take(n) for k, n in (("t10", B * Lo), ("p10", B * Lo), ("n10", B), ("nk", B), ("order", B * Fu), ("rank", B * Fu), ("Ot", B * Tm * 15),
                                 ("Op", B * Tm * 15), ("Sp", B * Tm * 257 * 2), ("dOp", B * Tm * 15), ("dfr", B * Tm * 256), ("dp10", B * Lo))}  # (+ cw, dw behind)
    return dict(nk=ws[o["nk"]:o["nk"] + B].view(torch.int32), n10=ws[o["n10"]:o["n10"] + B].view(torch.int32),
                Ot=ws[o["Ot"]:o["Ot"] + B * Tm * 15].view(B, Tm, 15), Op=ws[o["Op"]:o["Op"] + B * Tm * 15].view(B, Tm, 15),
                dOp=ws[o["dOp"]:o["dOp"] + B * Tm * 15].view(B, Tm, 15), dp10=ws[o["dp10"]:o["dp10"] + B * Lo].view(B, Lo),
                p10=ws[o["p10"]:o["p10"] + B * Lo].view(B, Lo), t10=ws[o["t10"]:o["t10"] + B * Lo].view(B, Lo))


def stoi_loss(y_true_batch, y_pred_batch, lens, reduction="mean"):
    """utility.stoi_loss: -STOI of the enhanced waveform against the clean one (batch mean, or per utterance for
    reduction != "mean").  Stays on the device of `y_pred_batch`; gradients flow to `y_pred_batch`."""
    y_pred_batch = torch.squeeze(y_pred_batch, dim=-1) if y_pred_batch.dim() == 3 else y_pred_batch
    y_true_batch = torch.squeeze(y_true_batch, dim=-1) if y_true_batch.dim() == 3 else y_true_batch
    B, L = y_pred_batch.shape
    lens_t = _lens_tensor(lens, B, L, y_pred_batch.device)
    if STOI_KERNELS and y_pred_batch.is_cuda and (L * 5 + 7) // 8 >= 256:
        D = _StoiHip.apply(y_true_batch.to(y_pred_batch.device), y_pred_batch, lens_t)
    else:
        D = _stoi_d(y_true_batch.to(y_pred_batch.device), y_pred_batch, lens_t)
    return -D.mean() if reduction == "mean" else -D


def compute_loss(source, pred_source, length):
    """TemporalCRN.compute_loss (CRN.py:593-617): (loss, stoi, sisnr) with loss = 0.7 * stoi + 0.3 * sisnr, sisnr = -SI-SNR;
    a NaN loss is replaced by zeros (CRN.py:613-616).  The reference also prints sisnr every call (CRN.py:612); dropped."""
    stoi = stoi_loss(source, pred_source, length)
    sisnr = -cal_si_snr(pred_source, source, length)
    loss = 0.7 * stoi + 0.3 * sisnr
    bad = torch.isnan(loss)
    zero = torch.zeros_like(loss)  # no gradient, like the reference's fill_(0.0)
    return torch.where(bad, zero, loss), torch.where(bad, zero, stoi), torch.where(bad, zero, sisnr)


# =====================================================================================================================
# PESQ loss (utility.py:615-814) and GTSA.compute_loss (GTSA.py:411-433)
# =====================================================================================================================
PESQ_MIN_SAMPLES = 4864  # 20 spectrogram frames (1 + L // 256): the shortest input the reference's 20-frame syllables have a value for
_PESQ_NB, _PESQ_NFFT, _PESQ_HOP, _PESQ_BINS = 49, 1024, 256, 513
_PESQ_LOW_F, _PESQ_HIGH_F = int(2 * 300 / 16000 * 513), int(2 * 3000 / 16000 * 513)  # level alignment over bins [19, 192)
_PESQ_SP, _PESQ_SL, _PESQ_ZWICKER = 6.910853e-1, 1.866055e-1, 0.23
# utility.py:668-710, the tables of ITU-T P.862 at 16 kHz: absolute hearing threshold, power density correction, band widths in Bark
_PESQ_ABS_THRESH = (
    51286152.000000, 2454709.500000, 70794.593750, 4897.788574, 1174.897705, 389.045166, 104.712860, 45.708820, 17.782795, 9.772372,
    4.897789, 3.090296, 1.905461, 1.258925, 0.977237, 0.724436, 0.562341, 0.457088, 0.389045, 0.331131, 0.295121, 0.269153, 0.257040,
    0.251189, 0.251189, 0.251189, 0.251189, 0.263027, 0.288403, 0.309030, 0.338844, 0.371535, 0.398107, 0.436516, 0.467735, 0.489779,
    0.501187, 0.501187, 0.512861, 0.524807, 0.524807, 0.524807, 0.512861, 0.478630, 0.426580, 0.371535, 0.363078, 0.416869, 0.537032)
_PESQ_POW_DENS = (
    100.000000, 99.999992, 100.000000, 100.000008, 100.000008, 100.000015, 99.999992, 99.999969, 50.000027, 100.000000, 99.999969,
    100.000015, 99.999947, 100.000061, 53.047077, 110.000046, 117.991989, 65.000000, 68.760147, 69.999931, 71.428818, 75.000038,
    76.843384, 80.968781, 88.646126, 63.864388, 68.155350, 72.547775, 75.584831, 58.379192, 80.950836, 64.135651, 54.384785, 73.821884,
    64.437073, 59.176456, 65.521278, 61.399822, 58.144047, 57.004543, 64.126297, 54.311001, 61.114979, 55.077751, 56.849335, 55.628868,
    53.137054, 54.985844, 79.546974)
_PESQ_ZW_H = (2.00, 2.00, 2.00, 2.00, 1.82, 1.66, 1.51, 1.39, 1.29, 1.20, 1.12, 1.05) + (1.00,) * 37
_PESQ_WIDTH = (
    0.157344, 0.317994, 0.322441, 0.326934, 0.331474, 0.336061, 0.340697, 0.345381, 0.350114, 0.354897, 0.359729, 0.364611, 0.369544,
    0.374529, 0.379565, 0.384653, 0.389794, 0.394989, 0.400236, 0.405538, 0.410894, 0.416306, 0.421773, 0.427297, 0.432877, 0.438514,
    0.444209, 0.449962, 0.455774, 0.461645, 0.467577, 0.473569, 0.479621, 0.485736, 0.491912, 0.498151, 0.504454, 0.510819, 0.517250,
    0.523745, 0.530308, 0.536934, 0.543629, 0.550390, 0.557220, 0.564119, 0.571085, 0.578125, 0.585232)


def _pesq_band_edges():
    """The 50 integer bin edges of the 49 Bark bands (bark2hz, utility.py:639-648); neighbours may coincide (an empty band)."""
    edges = []
    for z in np.linspace(0, 21, _PESQ_NB + 1):
        if z < 2:
            z = (z - 0.3) / 0.85
        elif z > 20.1:
            z = (z + 4.422) / 1.22
        edges.append(int(2 * (1960 * (z + 0.53) / (26.28 - z)) / 16000 * _PESQ_BINS))
    return edges


_PESQ_PLAN = {}


def _pesq_plan(device):
    """Per-device tables, built once.  All of them are the float32 numbers the reference's float32 tensors hold; a float64 run of
    `_pesq_d` widens those, so it is the exact value of the function the float32 reference rounds."""
    key = str(device)
    if key not in _PESQ_PLAN:
        f32 = np.float32
        edges = _pesq_band_edges()
        thr = np.asarray(_PESQ_ABS_THRESH, f32) * f32(1e4)
        zp = (np.asarray(_PESQ_ZW_H, f32) ** f32(0.15) * f32(_PESQ_ZWICKER)).astype(f32)
        win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(512) / 512)).astype(f32)  # periodic Hann(512), centred in 1024 points
        bandmat = np.zeros((_PESQ_NB, _PESQ_BINS), f32)
        band_of = np.full(_PESQ_BINS, -1, np.int32)
        for j in range(_PESQ_NB):
            bandmat[j, edges[j]:edges[j + 1]] = 1
            band_of[edges[j]:edges[j + 1]] = j
        cfac = (np.asarray(_PESQ_POW_DENS, f32) * f32(_PESQ_SP)).astype(f32)
        k2 = ((f32(2) * thr) ** zp).astype(f32)
        width = np.asarray(_PESQ_WIDTH, f32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        _PESQ_PLAN[key] = dict(edges=edges, thr=t(thr), zp=t(zp), win=t(win), bandmat=t(bandmat), cfac=t(cfac), k2=t(k2), width=t(width),
                               # tables of the kernel form (csrc/se_pesq.hip): band edges [50], bin -> band [513], [5][49] band constants
                               edges_dev=t(np.asarray(edges, np.int32)), band_of=t(band_of),
                               band_tab=t(np.stack([cfac, thr, zp, k2, width]).astype(f32)))
    return _PESQ_PLAN[key]


def _pesq_d(y_true, y_pred, lens, margins=None):
    """-PESQ-like score of utility.py:723-814 for every row at once: [B] values on the inputs' device, in the inputs' dtype (float32
    or float64), differentiable w.r.t. y_pred.  Row b is the reference's value for y[b, :lens[b]] run alone: reflect padding at the
    row's own end, nothing at or beyond lens[b] is read (NaN there is harmless).  A row with fewer than 20 frames (lens[b] < 4864)
    yields NaN with a zero gradient.  The CPU path and the checker of the se_loss_pesq_* kernels (PESQ_KERNELS = False).

    `margins`, a dict, receives per branch family the smallest relative distance of any comparison from its threshold (the fixture
    maker's condition that float32 and float64 take the same branches)."""
    dev, dt = y_pred.device, y_pred.dtype
    P = _pesq_plan(dev)
    y_true = y_true.detach().to(dt)
    B, L = y_pred.shape
    Tm = 1 + L // _PESQ_HOP
    Tb = 1 + torch.div(lens, _PESQ_HOP, rounding_mode="floor")
    bad = Tb < 20
    Tb = torch.where(bad, torch.full_like(Tb, 20), Tb)
    tv = (torch.arange(Tm, device=dev)[None, :] < Tb[:, None]) & ~bad[:, None]  # [B, Tm]
    Tf = Tb.to(dt)
    thr, zp, k2, w = (P[k].to(dt)[None, :, None] for k in ("thr", "zp", "k2", "width"))
    cfac = P["cfac"].to(dt)[None, :, None]
    # ---- Spectrogram(1024, 512, 256, power=2): the 512 samples under the window, gathered through the reflect rule of the row's own end
    n = (torch.arange(Tm, device=dev) * _PESQ_HOP - 256)[:, None] + torch.arange(512, device=dev)[None, :]  # [Tm, 512]
    m = n.abs()[None]
    ln = lens[:, None, None]
    m = torch.where(m >= ln, 2 * (ln - 1) - m, m).clamp(0, L - 1)  # [B, Tm, 512]

    def bands(y):
        fr = torch.gather(y, 1, m.reshape(B, -1)).reshape(B, Tm, 512)
        fr = torch.where(tv[..., None], fr, torch.zeros_like(fr)) * P["win"].to(dt)
        S = torch.fft.rfft(Fn.pad(fr, (256, 256)), dim=-1)
        pw = S.real ** 2 + S.imag ** 2  # [B, Tm, 513], zero beyond the row's frames
        level = pw[..., _PESQ_LOW_F:_PESQ_HIGH_F].sum((1, 2)) / ((_PESQ_HIGH_F - _PESQ_LOW_F) * Tf) + 1e-14
        raw = (pw @ P["bandmat"].to(dt).T).transpose(1, 2)  # [B, 49, Tm]
        return raw * (1e7 / level)[:, None, None] * cfac

    def note(name, x, c, sel=None):
        if margins is not None:  # x [B, 49, Tm] or [B, Tm] against the threshold c, over the rows' own frames
            r = (x.detach() - c).abs() / c
            ok = tv[:, None, :].expand_as(r) if r.dim() == 3 else tv
            r = r[ok if sel is None else ok & sel]
            if r.numel():
                margins[name] = min(margins.get(name, float("inf")), float(r.min()))

    Bt, Bp = bands(y_true), bands(y_pred)
    tvb = tv[:, None, :]
    mt = (Bt > thr).to(dt)
    mp = (Bp > thr).to(dt)
    note("band_true", Bt, thr)
    note("band_pred", Bp, thr)
    tt = (Bt * mt).sum(1)
    note("silence", tt, 1e7)
    ns = (tt > 1e7).to(dt)[:, None, :]
    # ---- band equalisation of the clean signal by the ratio of time means
    at = (Bt * mt * ns).sum(2, keepdim=True) / Tf[:, None, None]
    ap = (Bp * mp * ns).sum(2, keepdim=True) / Tf[:, None, None]
    eq = (ap + 1e3) / (at + 1e3)
    if margins is not None:
        for c in (0.01, 100.0):
            margins["eq_clamp"] = min(margins.get("eq_clamp", float("inf")), float(((eq.detach() - c).abs() / c)[~bad].min()))
    eq = torch.clamp(eq, 0.01, 100)
    Bt = Bt * eq
    mt = (Bt > thr).to(dt)
    note("band_true_eq", Bt, thr)
    tt = (Bt * mt).sum(1)
    tp = (Bp * mp).sum(1)
    # ---- time recurrence s_t = 0.2 s_{t-1} + (total_true_t + 5e3) / (total_pred_t + 5e3), s_{-1} = 1
    r = (tt + 5e3) / (tp + 5e3)
    s, ss = torch.ones(B, dtype=dt, device=dev), []
    for t in range(Tm):
        s = 0.2 * s + r[:, t]
        ss.append(s)
    s = torch.stack(ss, 1)
    note("s_lo", s, 3e-4)
    note("s_hi", s, 5.0)
    Bp = Bp * torch.clamp(s, 3e-4, 5.0)[:, None, :]
    # ---- loudness (Zwicker), disturbances
    Lp = k2 * ((0.5 + 0.5 * Bp / thr) ** zp - 1) * mp * _PESQ_SL
    Lt = k2 * ((0.5 + 0.5 * Bt / thr) ** zp - 1) * mt * _PESQ_SL
    d = Lp - Lt
    mm = torch.where(Lp < Lt, Lp, Lt) * 0.25
    live = ((d != 0) | (mm != 0)).detach()  # both loudnesses exactly zero: 0 > 0 is false in every arithmetic
    if margins is not None:
        sc = torch.maximum(d.detach().abs(), mm.detach().abs()).clamp(min=1e-300)
        for name, x in (("dead_hi", d - mm), ("dead_lo", d + mm)):
            rr = (x.detach().abs() / sc)[live & tvb.expand_as(live)]
            if rr.numel():
                margins[name] = min(margins.get(name, float("inf")), float(rr.min()))
    zero = torch.zeros_like(d)
    dist = torch.where(d > mm, d - mm, zero) + torch.where(d < -mm, d + mm, zero)
    wsum = w.sum()
    sym = ((dist.abs() * w) ** 2).sum(1) / wsum
    sym = sym ** 0.5 * wsum
    h = ((Lp + 50) / (Lt + 50)) ** 1.2
    moved = (dist != 0).detach()  # the asymmetry factor multiplies the disturbance: where that is zero its branch decides nothing
    note("asym_3", h, 3.0, moved)
    note("asym_12", h, 12.0, moved)
    h = torch.clamp(torch.where(h < 3, torch.zeros_like(h), h), 0, 12)
    asym = ((dist * h).abs() * w).sum(1) / wsum
    asym = asym * wsum
    hh = ((tt + 1e5) / 1e7) ** 0.04
    note("cap_sym", sym / hh, 45.0)
    note("cap_asym", asym / hh, 45.0)
    sym = torch.clamp(sym / hh, max=45.0)
    asym = torch.clamp(asym / hh, max=45.0)
    # ---- syllables of 20 frames every 10 (power-6 mean) and the tail block of the last `left` frames; power-2 mean over them
    nb = torch.div(Tb - 20, 10, rounding_mode="floor") + 1
    left = Tb - 10 * nb
    ti = torch.arange(Tm, device=dev)[None, :]
    tail = (ti >= (Tb - left)[:, None]) & (ti < Tb[:, None])
    kvalid = torch.arange((Tm - 20) // 10 + 1, device=dev)[None, :] < nb[:, None]

    def aggregate(x):
        x6 = x ** 6
        blocks = x6.unfold(1, 20, 10).mean(-1)  # [B, NBm]
        last = torch.where(tail, x6, torch.zeros_like(x6)).sum(1) / left.to(dt)
        blocks = (blocks + 1e-8) ** (1.0 / 6)
        last = (last + 1e-8) ** (1.0 / 6)
        tot = torch.where(kvalid, blocks ** 2, torch.zeros_like(blocks)).sum(1) + last ** 2
        return (tot / (nb + 1).to(dt) + 1e-8) ** 0.5

    res = 4.5 - 0.1 * aggregate(sym) - 0.0309 * aggregate(asym)
    return torch.where(bad, torch.full_like(res, float("nan")), -res)


PESQ_KERNELS = True  # CUDA tensors: csrc/se_pesq.hip (2 launches forward, 3 backward); False: the batched torch restatement _pesq_d, the checker


class _PesqHip(torch.autograd.Function):
    """Per-row value of utility.py:723-814 on the se_loss_pesq_* kernels; gradient to the prediction only."""

    @staticmethod
    def forward(ctx, y_true, y_pred, lens):
        from . import engine as _engine
        lib = _engine.load_library()
        P = _pesq_plan(y_pred.device)
        B, L = y_pred.shape
        yt, yp, ln = y_true.detach().contiguous().float(), y_pred.detach().contiguous().float(), lens.contiguous().to(torch.int64)
        ws = torch.empty(int(lib.se_loss_pesq_ws_floats(B, L)), dtype=torch.float32, device=y_pred.device)
        val = torch.empty(B, dtype=torch.float32, device=y_pred.device)
        st = C.c_void_p(torch.cuda.current_stream(y_pred.device).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if lib.se_loss_pesq_fwd(p(yt), p(yp), p(ln), B, L, p(P["win"]), p(P["edges_dev"]), p(P["band_tab"]), p(ws), p(val), st):
            raise RuntimeError(lib.se_loss_pesq_last_error().decode())
        ctx.save_for_backward(ln, ws)
        ctx.shape = (B, L)
        ctx.dev = y_pred.device
        return val

    @staticmethod
    def backward(ctx, gv):
        from . import engine as _engine
        lib = _engine.load_library()
        ln, ws = ctx.saved_tensors
        B, L = ctx.shape
        P = _pesq_plan(ctx.dev)
        g = gv.contiguous().float()
        dpred = torch.empty(B, L, dtype=torch.float32, device=ctx.dev)
        st = C.c_void_p(torch.cuda.current_stream(ctx.dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if lib.se_loss_pesq_bwd(p(g), p(ln), B, L, p(P["win"]), p(P["band_of"]), p(P["band_tab"]), p(ws), p(dpred), st):
            raise RuntimeError(lib.se_loss_pesq_last_error().decode())
        return None, dpred, None


def pesq_loss(y_true_batch, y_pred_batch, lens=None, reduction="mean"):
    """utility.pesq_loss (utility.py:615-814): minus the differentiable PESQ-like score of the enhanced waveform against the clean one.
    Row b is the reference's value for y[b, :lens[b]] run ALONE (reflect padding at the row's own end; samples at or beyond lens[b]
    are never read); "mean" returns the batch mean, anything else the per-row vector; lens=None means the full rows.  Gradients
    flow to `y_pred_batch` only.  Stays on the device of `y_pred_batch`: the se_loss_pesq_* kernels on GPU tensors, `_pesq_d` else.

    Deviations from the reference, on purpose: it ignores `lens`; at B > 1 it reuses the name `h` across its loop over the batch and
    fails with a shape error unless T is 49, and would return the last row's value only.  Where it has a value (B = 1, lens[0] = L)
    this one equals it.  Fewer than 20 spectrogram frames (4864 samples) have no value there (its 20-frame unfold raises): refused
    here with NotImplementedError, for L and for `lens` given on the host; `lens` on the device is not synchronised on, such a row
    yields NaN with a zero gradient.  The kernels hold a row's frames in LDS: rows of more than 896 frames (14.3 s) raise RuntimeError
    on GPU tensors (PESQ_KERNELS = False runs them on the restatement)."""
    y_pred_batch = torch.squeeze(y_pred_batch, dim=-1) if y_pred_batch.dim() == 3 else y_pred_batch
    y_true_batch = torch.squeeze(y_true_batch, dim=-1) if y_true_batch.dim() == 3 else y_true_batch
    B, L = y_pred_batch.shape
    host_lens = lens is not None and not (torch.is_tensor(lens) and lens.is_cuda)
    if L < PESQ_MIN_SAMPLES or (host_lens and int(torch.as_tensor(lens).min()) < PESQ_MIN_SAMPLES):
        raise NotImplementedError(f"pesq_loss has no value for fewer than 20 spectrogram frames ({PESQ_MIN_SAMPLES} samples); "
                                  f"got L = {L}, lens = {None if lens is None else [int(v) for v in torch.as_tensor(lens).reshape(-1)] if host_lens else 'on device'}")
    lens_t = _lens_tensor(lens, B, L, y_pred_batch.device)
    if PESQ_KERNELS and y_pred_batch.is_cuda:
        v = _PesqHip.apply(y_true_batch.to(y_pred_batch.device), y_pred_batch, lens_t)
    else:
        v = _pesq_d(y_true_batch.to(y_pred_batch.device), y_pred_batch, lens_t)
    return v.mean() if reduction == "mean" else v


def gtsa_compute_loss(source, pred_source, length):
    """GTSA.compute_loss (GTSA.py:411-433): (loss, mae, sisnr) with loss = 0.7 * pesq_loss + 0.3 * sisnr, sisnr = -SI-SNR; a NaN loss
    is replaced by zeros without a gradient, all three (GTSA.py:429-432).  The reference's print of sisnr is dropped."""
    mae = pesq_loss(source, pred_source, length)
    sisnr = -cal_si_snr(pred_source, source, length)
    loss = 0.7 * mae + 0.3 * sisnr
    bad = torch.isnan(loss)
    zero = torch.zeros_like(loss)
    return torch.where(bad, zero, loss), torch.where(bad, zero, mae), torch.where(bad, zero, sisnr)


# =====================================================================================================================
# HiFi-GAN spectral loss (Hifi-GAN/hifigan.py:986-1013)
# =====================================================================================================================
def stft_loss(pred, real, nfft=400, nhop=200, nwin=200, window="hann_window", phase=False):
    """Hifi_GAN.stft_loss on torch.stft(..., return_complex=True): the reference's legacy real-view call is centred, reflect-padded,
    one-sided and unnormalised, the window centred in nfft.  |X| = sqrt(clamp(re^2 + im^2, 1e-14)).  phase=True: 0.7 * the mean
    absolute difference of |X|^0.3 + 0.3 * that of |X|^0.3 * X / |X| (real and imaginary parts alike); else the mean absolute
    difference of log |X|.  Plus the spectral convergence ||P - R||_F / ||P||_F over the WHOLE batch (on the 0.3-power magnitudes
    when phase=True, as the reference reuses the name).  Plain torch, differentiable, on the inputs' device."""
    if pred.dim() > 2:
        pred = pred.squeeze(1)
    if real.dim() > 2:
        real = real.squeeze(1)
    win = getattr(torch, window)(nwin).to(device=pred.device, dtype=pred.dtype)

    def spec(x):
        s = torch.view_as_real(torch.stft(x, nfft, nhop, nwin, win, center=True, pad_mode="reflect", normalized=False, onesided=True,
                                          return_complex=True))
        return s, torch.sqrt(torch.clamp(s[..., 0] ** 2 + s[..., 1] ** 2, min=1e-14)).unsqueeze(-1)
    (ps, pm), (rs, rm) = spec(pred), spec(real)
    if phase:
        pp, rp = ps / pm, rs / rm
        pm, rm = pm ** 0.3, rm ** 0.3
        first = 0.7 * torch.mean(torch.abs(pm - rm)) + 0.3 * torch.mean(torch.abs(pm * pp - rm * rp))
    else:
        first = torch.mean(torch.abs(torch.log(pm) - torch.log(rm)))
    return first + torch.linalg.norm(pm - rm) / torch.linalg.norm(pm)
