"""The passes that every model's kernel path shares, one definition each, on the launch layer of train_ops.py (`conv_w`, `wgrad`,
`gemm_tn`, `colsum3`, `colsum_tall`, `_new`, `_p`, `_run`: re-exported here): the call geometry, the signal chain (STFT in,
iSTFT + overlap-add out, and its adjoint), the plain U-Net encoder block, the
U-Net decoder and one GRU layer of the backward sweep.  train_net.CRNFunction, general_beamformer (inference and GBFFunction) and
fsn_training.FSNFunction are orchestration over these.  Layout: S = N segments x B utterances, SEGMENT-major, activations
[S][C][T][F]; an encoder block's input is [N + 1][B][C][T][F] with the carried time history in slab 0 (`xprev = x - one slab`).
Every launch goes through `_run` (events when train_ops.PROF is set).  Nothing here keeps a tensor alive beyond what it returns.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import train_ops as K
from .train_ops import _new, _p, _run, colsum3, colsum_tall, conv_w, gemm_tn, wgrad  # noqa: F401  (re-exported)

_sig_cache = {}


def _as_flag(flag):
    """realtime_process's flag: a bool, or the trainer's per-utterance flag tensor (data['flag'], shape [B]; one value per batch)."""
    return bool(flag.reshape(-1)[0].item()) if isinstance(flag, torch.Tensor) else bool(flag)


def _as_flags(flag, B):
    """Per-utterance flags of a batch of chunk chains: a bool or ONE value (every utterance; the reference trainer's flag tensor at
    batch 1), or B values as a list or the trainer's flag tensor (read once, here).  -> a list of B bools; a mixed tensor stays mixed."""
    if isinstance(flag, torch.Tensor):
        flag = flag.reshape(-1).tolist()
    if isinstance(flag, (list, tuple)):
        if len(flag) == 1:
            return [bool(flag[0])] * B
        if len(flag) != B:
            raise ValueError(f"{len(flag)} flags for a batch of {B} utterances")
        return [bool(f) for f in flag]
    return [bool(flag)] * B


def _as_lengths(lengths, B, Lmax):
    """Per-utterance lengths (a list or an integer tensor, read once, here; None: every utterance is Lmax long) -> a list of B ints"""
    if lengths is None:
        return [int(Lmax)] * B
    lengths = [int(v) for v in (lengths.reshape(-1).tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(lengths) != B or min(lengths) < 1 or max(lengths) > Lmax:
        raise ValueError(f"lengths must be {B} values in [1, {Lmax}], got {lengths}")
    return lengths


def segment_geometry(L, flag, segment_length, hop, n_fft, ch=()):
    """One realtime_process call over L samples in half-overlapping segments (utility.segmentation); flag=False pads P = Ks / 2 samples
    on the left and strips them again.  ch = the U-Net levels' channels, input first; Fq[i] = level i's frequency size (stride 2)."""
    Ks = segment_length
    P = Ks // 2
    Lp = L if flag else L + P
    gap = Ks - (P + Lp % Ks) % Ks
    Fq = [n_fft // 2 + 1]
    for _ in ch[1:]:
        Fq.append((Fq[-1] - 1) // 2 + 1)
    return dict(L=L, Ks=Ks, P=P, Lp=Lp, gap=gap, N=2 * (Lp + gap + P) // Ks, off0=-P if flag else -2 * P, skip=0 if flag else P,
                T=1 + Ks // hop, F0=Fq[0], ch=list(ch), Fq=Fq)


def ragged_geometry(lengths, flags, segment_length, hop, n_fft, ch=()):
    """A batch of chunk chains in one call: utterance b is lengths[b] samples long and continues its own state iff flags[b].  Segment
    positions do not depend on the length, so every utterance keeps the geometry it would have alone: Lp, gap, Nb, off0, skip are lists,
    entry b = segment_geometry(lengths[b], flags[b], ...); N = max Nb segments are run, L = max length is the width of the batch."""
    per = [segment_geometry(int(L), bool(f), segment_length, hop, n_fft, ch) for L, f in zip(lengths, flags)]
    q = dict(per[0])
    q.update(L=max(p["L"] for p in per), N=max(p["N"] for p in per), lengths=[p["L"] for p in per], flags=[bool(f) for f in flags],
             Nb=[p["N"] for p in per], **{k: [p[k] for p in per] for k in ("Lp", "gap", "off0", "skip")})
    return q


def grads_in_parameter_order(model, grads):
    """{name: gradient} -> the gradients in named_parameters() order (None where there is none); `net.0` aliases `conv`."""
    named = ((grads.get(name.replace(".net.0.", ".conv.")), p) for name, p in model.named_parameters())
    return [None if gr is None else gr.reshape(p.shape) for gr, p in named]


def _sig(dev, n_fft, win, hop, seg):
    key = (dev.index, n_fft, win, hop, seg)
    if key not in _sig_cache:
        h = C.c_void_p()
        K._chk(K._lib().se_sig_create(n_fft, win, hop, seg, dev.index or 0, C.byref(h)))
        _sig_cache[key] = h
    return _sig_cache[key]


def gln_fwd(x, xs, y_ptr, ys, w, b, S, Cc, T, Fi, Fo, mode, act, eps_mode=0):
    stats = _new(S, 2, dev=w.device)
    _run("k_tgln_fwd", 0.0, K._lib().se_train_gln_fwd, _p(x), *xs, y_ptr, *ys, _p(w), _p(b), _p(stats), S, Cc, T, Fi, Fo, mode, act, eps_mode, K._st())
    return stats


def gln_bwd(dy_ptr, ds, x, xs, w, stats, S, Cc, T, Fi, mode, act, eps_mode=0):
    """-> dx (same shape / strides as x), dw, db, dpre (column sums of the [S][NA] slabs)"""
    NA = Cc * Fi if mode else Cc
    dev = x.device
    dx = torch.empty_like(x)
    parts = [_new(S, NA, dev=dev) for _ in range(3)]
    _run("k_tgln_bwd", 0.0, K._lib().se_train_gln_bwd, dy_ptr, *ds, _p(x), *xs, _p(dx), _p(w), _p(stats), _p(parts[0]), _p(parts[1]), _p(parts[2]),
         S, Cc, T, Fi, mode, act, eps_mode, K._st())
    dw, db, dpre = colsum3(S, (parts[0], NA), (parts[1], NA), (parts[2], NA))
    return dx, dw, db, dpre


def transpose(w):
    """[R, C] -> [C, R] contiguous (weights only: tiny)."""
    return w.t().contiguous()


def _cs(Cc, T, Fq):
    """(channel, time, frequency-row) strides of a contiguous [S][C][T][F] tensor, as gln_fwd / gln_bwd take them"""
    return (Cc * T * Fq, T * Fq, Fq)


# ---- signal chain ----------------------------------------------------------------------------------------------------------------
def stft(sig, x, B, M, L, off0, P, N, T, F0):
    """x [B][M][L] -> spec [N][B*M][T][F0][2]: segment n of every row starts at sample off0 + n * P (zeros outside [0, L))."""
    spec = _new(N, B * M, T, F0, 2, dev=x.device)
    _run("k_stft", 0.0, K._lib().se_sig_stft, sig, _p(x), B, M, L, off0, P, N, _p(spec), K._st())
    return spec


def _rows(values, dev):
    """host ints -> a device int64 [B] (one asynchronous copy; the row kernels read it on the stream)"""
    return torch.tensor(values, dtype=torch.int64).to(dev, non_blocking=True)


def stft_rows(sig, x, B, M, Lmax, off0, lens, P, N, T, F0):
    """stft for a batch of chunk chains: off0 / lens = device int64 [B]; utterance b is zero outside [0, lens[b]) whatever x holds there"""
    spec = _new(N, B * M, T, F0, 2, dev=x.device)
    _run("k_stft", 0.0, K._lib().se_sig_stft_rows, sig, _p(x), B, M, Lmax, C.c_void_p(off0.data_ptr()), C.c_void_p(lens.data_ptr()), P, N, _p(spec), K._st())
    return spec


def slab_gather(src, idx, B, X, sN, sB, off_floats=0, dst=None):
    """dst [B][X] (new unless given): dst[b] = the X floats of src at off_floats + idx[b] * sN + b * sB, zeros where idx[b] < 0 (idx:
    device int64 [B])"""
    if dst is None:
        dst = _new(B, X, dev=src.device)
    _run("k_slab_gather", 0.0, K._lib().se_train_slab_gather, _p(src, off_floats), C.c_void_p(idx.data_ptr()), _p(dst), B, X, sN, sB, K._st())
    return dst


def input_features(spec, x_full, S, B, M, C0, T, F0, atan2=0):
    """spec -> magnitude + phase-difference features into slabs 1.. of x_full [N + 1][B][C0][T][F0]"""
    _run("k_tfeat", 0.0, K._lib().se_train_feat, _p(spec), _p(x_full, B * C0 * T * F0), S, M, T, F0, atan2, K._st())


def istft(sig, Y, yseg, row0=0):
    """Y [S][T][F0][2] -> rows row0 .. row0 + S of yseg [.., Ks]"""
    _run("k_istft", 0.0, K._lib().se_sig_istft, sig, _p(Y), Y.shape[0], _p(yseg, row0 * yseg.shape[-1]), K._st())


def overlap_add(sig, yseg, B, Lout, skip):
    """utility.over_add of the segment-major yseg [N*B][Ks] -> pred [B][Lout], the first `skip` samples dropped"""
    pred = _new(B, Lout, dev=yseg.device)
    _run("k_tola", 0.0, K._lib().se_train_ola_fwd, sig, _p(yseg), _p(pred), B, Lout, skip, K._st())
    return pred


def synthesis(sig, Y, B, Ks, Lout, skip):
    """Y [S][T][F0][2] -> pred [B][Lout]: iSTFT of every segment, then overlap-add"""
    yseg = _new(Y.shape[0], Ks, dev=Y.device)
    istft(sig, Y, yseg)
    return overlap_add(sig, yseg, B, Lout, skip)


def synthesis_adjoint(sig, dpred, B, N, Lout, skip, Ks, T, F0):
    """dpred [B][Lout] -> dY [S][T][F0][2]: the adjoint of overlap-add, then of the iSTFT (an STFT of every segment)"""
    gseg = _new(N * B, Ks, dev=dpred.device)
    _run("k_tola", 0.0, K._lib().se_train_ola_bwd, sig, _p(dpred), _p(gseg), B, N, Lout, skip, K._st())
    return stft(sig, gseg, N * B, 1, Ks, 0, 0, 1, T, F0).view(N * B, T, F0, 2)


def synthesis_rows(sig, Y, B, Ks, Lmax, skip, lens):
    """synthesis for a batch of chunk chains: skip / lens = device int64 [B]; pred [B][Lmax] with pred[b][lens[b]:] = 0"""
    yseg = _new(Y.shape[0], Ks, dev=Y.device)
    istft(sig, Y, yseg)
    pred = _new(B, Lmax, dev=Y.device)
    _run("k_tola", 0.0, K._lib().se_train_ola_fwd_rows, sig, _p(yseg), _p(pred), B, Lmax, C.c_void_p(skip.data_ptr()), C.c_void_p(lens.data_ptr()), K._st())
    return pred


def synthesis_adjoint_rows(sig, dpred, B, N, Lmax, skip, lens, Ks, T, F0):
    """synthesis_adjoint for a batch of chunk chains; dpred[b][lens[b]:] is ignored"""
    gseg = _new(N * B, Ks, dev=dpred.device)
    _run("k_tola", 0.0, K._lib().se_train_ola_bwd_rows, sig, _p(dpred), _p(gseg), B, N, Lmax, C.c_void_p(skip.data_ptr()), C.c_void_p(lens.data_ptr()), K._st())
    return stft(sig, gseg, N * B, 1, Ks, 0, 0, 1, T, F0).view(N * B, T, F0, 2)


# ---- U-Net encoder block, plain variant: conv + gLN + ReLU ------------------------------------------------------------------------
def encoder_block_fwd(blk, x_full, y_ptr, ys, S, B, Ci, Co, T, Fi, Fo, d, eps_mode=0):
    """x_full [N + 1][B][Ci][T][Fi] -> gLN(ReLU(conv)) written at y_ptr with strides ys.  -> (pre-activation y, gLN statistics)"""
    y = _new(S, Co, T, Fo, dev=x_full.device)
    conv_w(0, _p(x_full, B * Ci * T * Fi), _p(x_full), blk.conv.weight, Ci * 15, 15, blk.conv.bias, y, S, Ci, Co, T, Fi, Fo, d, 0)
    return y, gln_fwd(y, _cs(Co, T, Fo), y_ptr, ys, blk.norm.weight, blk.norm.bias, S, Co, T, Fo, Fo, 0, 1, eps_mode)


def encoder_conv_bwd(blk, pre, grads, dy, x_full, dres, zero_bias, S, B, Ci, Co, T, Fi, Fo, d, need_dx=True):
    """dy = d conv output: the weight gradient (slab 0 of x_full, a constant, enters it) and -> d block input (+ dres, its skip use)"""
    grads[pre + "conv.weight"] = wgrad(dy, _p(x_full, B * Ci * T * Fi), _p(x_full), S, Co, Ci, T, Fo, Fi, d, 15)
    if not need_dx:
        return None
    dxi = _new(S, Ci, T, Fi, dev=dy.device)
    for kind in (1, 2):
        conv_w(kind, _p(dy), None, blk.conv.weight, 15, Ci * 15, zero_bias, dxi, S, Co, Ci, T, Fo, Fi, d)
    if dres is not None:
        _run("k_tadd", 0.0, K._lib().se_train_add, _p(dxi), _p(dres), dxi.numel(), K._st())
    return dxi


def encoder_block_bwd(blk, pre, grads, dy_ptr, ds, y, stats, x_full, dres, zero_bias, S, B, Ci, Co, T, Fi, Fo, d, eps_mode=0, need_dx=True):
    """Backward of encoder_block_fwd; dy_ptr / ds address the gradient of its output.  -> the gradient of the block input"""
    dy, dw, db, dpre = gln_bwd(dy_ptr, ds, y, _cs(Co, T, Fo), blk.norm.weight, stats, S, Co, T, Fo, 0, 1, eps_mode)
    grads[pre + "norm.weight"], grads[pre + "norm.bias"], grads[pre + "conv.bias"] = dw, db, dpre
    return encoder_conv_bwd(blk, pre, grads, dy, x_full, dres, zero_bias, S, B, Ci, Co, T, Fi, Fo, d, need_dx)


# ---- U-Net decoder ---------------------------------------------------------------------------------------------------------------
def decoder_fwd(deconvlist, xin, ch, Fq, S, B, T, act, eps_mode, keep=True, stacked=True):
    """The whole decoder: per level two parity launches of the transposed convolution, gLN + activation and - all levels but the
    last - the gated skip with encoder input xin[k] (CRN.py:485: residuals[-2-j]) through the 1x1 residual / residualmask pair.
    stacked: the pair is ONE launch over the stacked weights [2 Co][Cr], else one launch per half (2 Co may exceed 128 GEMM rows).
    xin = the encoder blocks' inputs and, last, the decoder's input [S][C][T][F], which is POPPED: without keep (the records
    decoder_bwd needs, one dict per level) nothing holds a level's input once the next has run.  -> (last level's output, records)"""
    lib = K._lib()
    x_in = xin.pop()
    dev = x_in.device
    Lv = len(deconvlist)
    dec = []
    Ci, Fi = ch[Lv], Fq[Lv]
    for j, blk in enumerate(deconvlist):
        Co, d, Fy = blk.conv.weight.shape[1], 2 ** j, 2 * Fi - 1
        yd = _new(S, Co, T, Fy, dev=dev)
        for kind in (1, 2):
            conv_w(kind, _p(x_in), None, blk.conv.weight, 15, Co * 15, blk.conv.bias, yd, S, Ci, Co, T, Fi, Fy, d)
        rec = dict(x_in=x_in, yd=yd, Ci=Ci, Co=Co, Fi=Fi, Fy=Fy, d=d)
        if j < Lv - 1:
            k = Lv - 1 - j
            Cr, Fr = ch[k], Fq[k]
            if Fr < Fy or Cr != Co:
                raise RuntimeError("decoder / skip geometry outside the reference's (CRN.py:389-392 crop branch is never taken)")
            z = _new(S, Co, T, Fr, dev=dev)
            rec["st"] = gln_fwd(yd, _cs(Co, T, Fy), _p(z), _cs(Co, T, Fr), blk.norm.weight, blk.norm.bias, S, Co, T, Fy, Fr, 0, act, eps_mode)
            res = _p(xin[k], B * Cr * T * Fr)
            uv = _new(S, 2 * Co, T, Fr, dev=dev)   # residual | residualmask
            if stacked:
                wuv = rec["wuv"] = _new(2 * Co, Cr, dev=dev)
                buv = _new(2 * Co, dev=dev)
                wuv[:Co].copy_(blk.residual.weight.view(Co, Cr)); wuv[Co:].copy_(blk.residualmask.weight.view(Co, Cr))
                buv[:Co].copy_(blk.residual.bias); buv[Co:].copy_(blk.residualmask.bias)
                conv_w(3, res, None, wuv, Cr, 1, buv, uv, S, Cr, 2 * Co, T, Fr, Fr, 0)
            else:
                conv_w(3, res, None, blk.residual.weight, Cr, 1, blk.residual.bias, uv, S, Cr, Co, T, Fr, Fr, 0, 0, 2 * Co, 0)
                conv_w(3, res, None, blk.residualmask.weight, Cr, 1, blk.residualmask.bias, uv, S, Cr, Co, T, Fr, Fr, 0, 0, 2 * Co, Co)
            out = _new(S, Co, T, Fr, dev=dev)
            st_uv = _new(S, 2, dev=dev)
            _run("k_tskip_fwd", 0.0, lib.se_train_skip_fwd, _p(uv), _p(z), _p(blk.residualnorm.weight), _p(blk.residualnorm.bias), _p(out), _p(st_uv),
                 S, Co, T, Fr, act, eps_mode, K._st())
            rec.update(z=z, uv=uv, st_uv=st_uv, k=k, Cr=Cr, Fr=Fr)
            x_in, Ci, Fi = out, Co, Fr
        else:
            x_in = _new(S, Co, T, Fy, dev=dev)
            rec["st"] = gln_fwd(yd, _cs(Co, T, Fy), _p(x_in), _cs(Co, T, Fy), blk.norm.weight, blk.norm.bias, S, Co, T, Fy, Fy, 0, act, eps_mode)
        if keep:
            dec.append(rec)
    return x_in, dec


def decoder_bwd(deconvlist, dec, xin, dout, grads, zero_bias, S, B, T, act, eps_mode, stacked=True, hook=None):
    """Backward of decoder_fwd, last level first; dout = the gradient of its output.  hook(j, dyd, rec), if given, may add into dyd,
    the gradient of level j's transposed-convolution output, and then returns the new conv.bias gradient (else None).
    -> (the gradient of the decoder input, {k: the gradient that reaches encoder input xin[k] as a skip tensor})"""
    lib = K._lib()
    dev = dout.device
    Lv = len(deconvlist)
    dres = {}
    for j in range(Lv - 1, -1, -1):
        blk, rec = deconvlist[j], dec[j]
        Ci, Co, Fi, Fy, d = rec["Ci"], rec["Co"], rec["Fi"], rec["Fy"], rec["d"]
        pre = f"deconvlist.{j}."
        if j < Lv - 1:
            Cr, Fr, k = rec["Cr"], rec["Fr"], rec["k"]
            duv = _new(S, 2 * Co, T, Fr, dev=dev)
            dz = _new(S, Co, T, Fr, dev=dev)
            pw, pb, pbias = _new(S, Co, dev=dev), _new(S, Co, dev=dev), _new(S, 2 * Co, dev=dev)
            _run("k_tskip_bwd", 0.0, lib.se_train_skip_bwd, _p(dout), _p(rec["uv"]), _p(rec["z"]), _p(blk.residualnorm.weight), _p(blk.residualnorm.bias),
                 _p(rec["st_uv"]), _p(duv), _p(dz), _p(pw), _p(pb), _p(pbias), S, Co, T, Fr, act, eps_mode, K._st())
            dnw, dnb, dbuv = colsum3(S, (pw, Co), (pb, Co), (pbias, 2 * Co))
            grads[pre + "residualnorm.weight"], grads[pre + "residualnorm.bias"] = dnw, dnb
            grads[pre + "residual.bias"], grads[pre + "residualmask.bias"] = dbuv[:Co], dbuv[Co:]
            dwuv = wgrad(duv, _p(xin[k], B * Cr * T * Fr), None, S, 2 * Co, Cr, T, Fr, Fr, 0, 1).view(2 * Co, Cr)
            grads[pre + "residual.weight"], grads[pre + "residualmask.weight"] = dwuv[:Co], dwuv[Co:]
            wuv = rec["wuv"] if stacked else torch.cat([blk.residual.weight.detach().view(Co, Cr), blk.residualmask.weight.detach().view(Co, Cr)])
            dr = _new(S, Cr, T, Fr, dev=dev)
            conv_w(3, _p(duv), None, wuv, 1, Cr, zero_bias, dr, S, 2 * Co, Cr, T, Fr, Fr, 0)
            dres[k] = dr
            dy_ptr, ds = _p(dz), _cs(Co, T, Fr)
        else:
            dy_ptr, ds = _p(dout), _cs(Co, T, Fy)
        dyd, dw, db, dpre = gln_bwd(dy_ptr, ds, rec["yd"], _cs(Co, T, Fy), blk.norm.weight, rec["st"], S, Co, T, Fy, 0, act, eps_mode)
        hooked = hook(j, dyd, rec) if hook is not None else None
        grads[pre + "norm.weight"], grads[pre + "norm.bias"], grads[pre + "conv.bias"] = dw, db, dpre if hooked is None else hooked
        grads[pre + "conv.weight"] = wgrad(rec["x_in"], dyd, None, S, Ci, Co, T, Fi, Fy, d, 15)
        dout = _new(S, Ci, T, Fi, dev=dev)
        conv_w(0, _p(dyd), None, blk.conv.weight, Co * 15, 15, zero_bias, dout, S, Co, Ci, T, Fy, Fi, d)
    return dout, dres


# ---- GRU layer, backward ---------------------------------------------------------------------------------------------------------
def gru_layer_bwd(dlayer, out, gates, h0, x_l, w_ih, w_hh, pre, l, grads, streams, nseg, T, H, Tseg, ldN, ldB, tag=0, tmo=None, steps=None):
    """One GRU layer of the backward sweep.  out / gates / dlayer hold `streams` sequences of nseg * T steps, rows addressed like
    train_ops._gru_seq_fwd's (Tseg, ldN, ldB); h0 [streams][H] is the state the call started from.  The carried state is detached at
    every segment seam (CRN.py:281), so NOTHING flows back across a seam: the rows are already [streams * nseg][T], and the BPTT is
    ONE persistent launch over streams * nseg independent sequences of T steps, each entering at row 0 of its h_{t-1} block.
    w_ih: the weight the forward's input GEMM used (zero-padded columns included).  Gradients go to grads[pre + "weight_ih_l{l}"] ...
    tag: the scratch buffer's (train_ops._scratch); tmo: a list that receives the launch's time-out word.  steps (device int32
    [streams * nseg], T or 0 per sequence; rows [streams][nseg * T] only): the dead sequences are skipped - dlayer is not read there and
    their dgi / dgh rows are zeros, which is what the weight-gradient GEMMs and column sums over all rows need.  -> d x_l"""
    dev = out.device
    R, n = streams * nseg * T, streams * nseg
    hp = _new(R, H, dev=dev)
    _run("k_gru_hprev", 0.0, K._lib().se_train_gru_hprev, _p(out), _p(h0), _p(hp), streams, nseg * T, H, Tseg, ldN, ldB, K._st())
    h0seg = hp.view(n, T, H)[:, 0].contiguous()
    dgi, dgh = _new(R, 3 * H, dev=dev), _new(R, 3 * H, dev=dev)
    sc = K._gru_seq_bwd(dlayer, None, gates, out, h0seg, transpose(w_hh), dgi, dgh, n, T, H, T, 0, T, 0, tag, steps=steps)
    if tmo is not None:
        tmo.append(sc[:2].view(torch.int32)[1:2].clone())   # this launch's timeout word, before the next launch's memset
    grads[pre + f"weight_ih_l{l}"] = gemm_tn(dgi, x_l)
    grads[pre + f"weight_hh_l{l}"] = gemm_tn(dgh, hp)
    grads[pre + f"bias_ih_l{l}"] = colsum_tall(dgi)
    grads[pre + f"bias_hh_l{l}"] = colsum_tall(dgh)
    return K._gemm(dgi, transpose(w_ih))
