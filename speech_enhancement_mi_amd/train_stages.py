"""The passes that every model's kernel path shares, one definition each, on the launch layer of train_ops.py (`conv_w`, `wgrad`,
`gemm_tn`, `colsum3`, `colsum_tall`, `_new`, `_p`, `_run`: re-exported here): the signal chain (STFT in, iSTFT + overlap-add out, and its
adjoint) and the carried-state gathers, which take the call's CallPlan (call_plan.py: the call geometry and the flag / lengths parser,
re-exported here under the names they had) and pick the scalar kernel or its `_rows` twin, the plain U-Net encoder block, the
U-Net decoder and one GRU layer of the backward sweep.  train_net.CRNFunction, general_beamformer (inference and GBFFunction) and
fsn_training.FSNFunction are orchestration over these.  Layout: S = N segments x B utterances, SEGMENT-major, activations
[S][C][T][F]; an encoder block's input is [N + 1][B][C][T][F] with the carried time history in slab 0 (`xprev = x - one slab`).
Every launch goes through `_run` (events when train_ops.PROF is set).  Nothing here keeps a tensor alive beyond what it returns.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import train_ops as K
from .call_plan import CallPlan, call_plan, ragged_geometry, segment_geometry  # noqa: F401  (re-exported)
from .call_plan import as_flag as _as_flag, as_flags as _as_flags, as_lengths as _as_lengths  # noqa: F401  (the names callers know)
from .train_ops import _new, _p, _run, colsum3, colsum_tall, conv_w, gemm_tn, wgrad  # noqa: F401  (re-exported)

_sig_cache = {}


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


# ---- signal chain: every helper takes the call's CallPlan and launches the scalar kernel (uniform) or its `_rows` twin (chains) -----
def _rows(values, dev):
    """host ints -> a device int64 [B] (one asynchronous copy; the row kernels read it on the stream)"""
    return torch.tensor(values, dtype=torch.int64).to(dev, non_blocking=True)


def row_table(plan, dev, key):
    """plan.table(key) as a device int64 [B]: copied once per plan and device, kept on the plan"""
    if (dev, key) not in plan.dev:
        plan.dev[dev, key] = _rows(plan.table(key), dev)
    return plan.dev[dev, key]


def _ip(t):
    return C.c_void_p(t.data_ptr())


def _stft(sig, x, rows_, M, L, off0, P, N, T, F0):
    """x [rows_][M][L] -> spec [N][rows_*M][T][F0][2]: segment n of every row starts at sample off0 + n * P (zeros outside [0, L))."""
    spec = _new(N, rows_ * M, T, F0, 2, dev=x.device)
    _run("k_stft", 0.0, K._lib().se_sig_stft, sig, _p(x), rows_, M, L, off0, P, N, _p(spec), K._st())
    return spec


def stft(plan, sig, x, M, n0=0, Nc=None):
    """x [B][M][L] -> spec [Nc][B*M][T][F0][2], segments [n0, n0 + Nc) of the call (default: all N): segment n of utterance b starts at
    sample off0[b] + n * P; zeros outside [0, lengths[b]) whatever x holds there."""
    N = plan.N - n0 if Nc is None else Nc
    if plan.uniform:
        return _stft(sig, x, plan.B, M, plan.L, plan.off0 + n0 * plan.P, plan.P, N, plan.T, plan.F0)
    off0 = row_table(plan, x.device, "off0") if n0 == 0 else _rows([o + n0 * plan.P for o in plan.off0], x.device)
    spec = _new(N, plan.B * M, plan.T, plan.F0, 2, dev=x.device)
    _run("k_stft", 0.0, K._lib().se_sig_stft_rows, sig, _p(x), plan.B, M, plan.L, _ip(off0), _ip(row_table(plan, x.device, "len")), plan.P, N, _p(spec), K._st())
    return spec


def slab_gather(src, idx, B, X, sN, sB, off_floats=0, dst=None):
    """dst [B][X] (new unless given): dst[b] = the X floats of src at off_floats + idx[b] * sN + b * sB, zeros where idx[b] < 0 (idx:
    device int64 [B])"""
    if dst is None:
        dst = _new(B, X, dev=src.device)
    _run("k_slab_gather", 0.0, K._lib().se_train_slab_gather, _p(src, off_floats), _ip(idx), _p(dst), B, X, sN, sB, K._st())
    return dst


def start_rows(plan, t, dst=None):
    """The rows of the carried tensor t [B][...] a call starts from: t itself when uniform (the caller decides between it and zeros by
    plan.flag), else row b where flags[b] and zeros where utterance b starts afresh (a new tensor, or into dst)."""
    if plan.uniform:
        return t if dst is None else dst.copy_(t)
    X = t.numel() // plan.B
    return slab_gather(t, row_table(plan, t.device, "carry"), plan.B, X, plan.B * X, X, dst=dst).view(t.shape)


def own_last_slab(plan, t, counts=None, copy=False):
    """t [n + 1][B][...] -> [B][...]: the slab after utterance b's own last segment - slab n for all when uniform (a view of t unless
    copy), else slab Nb[b], or counts[b] (a device int64 [B]) where t holds a part of the call only."""
    if plan.uniform:
        return t[-1].clone() if copy else t[-1]
    X = t[0][0].numel()
    return slab_gather(t, row_table(plan, t.device, "last") if counts is None else counts, plan.B, X, plan.B * X, X).view(t.shape[1:])


def input_features(spec, x_full, S, B, M, C0, T, F0, atan2=0):
    """spec -> magnitude + phase-difference features into slabs 1.. of x_full [N + 1][B][C0][T][F0]"""
    _run("k_tfeat", 0.0, K._lib().se_train_feat, _p(spec), _p(x_full, B * C0 * T * F0), S, M, T, F0, atan2, K._st())


def istft(sig, Y, yseg, row0=0):
    """Y [S][T][F0][2] -> rows row0 .. row0 + S of yseg [.., Ks]"""
    _run("k_istft", 0.0, K._lib().se_sig_istft, sig, _p(Y), Y.shape[0], _p(yseg, row0 * yseg.shape[-1]), K._st())


def istft_into(plan, sig, Y, yseg, n0, Nc):
    """Y [Nc * plan.B][T][F0][2], windows [n0, n0 + Nc) of the plan's streams -> yseg [N][B'][Ks], B' >= plan.B: straight in where the
    pass is as wide as yseg, else (a prefix pass: yseg is window-major at the whole batch's stride) window by window"""
    B = plan.B
    if yseg.shape[1] == B:
        istft(sig, Y, yseg.view(-1, plan.Ks), n0 * B)
    else:
        part = _new(Nc, B, plan.Ks, dev=Y.device)
        istft(sig, Y, part.view(-1, plan.Ks))
        yseg[n0:n0 + Nc, :B].copy_(part)


def overlap_add(plan, sig, yseg):
    """utility.over_add of the segment-major yseg [N*B][Ks] -> pred [B][L]: the first skip[b] samples dropped, pred[b][lengths[b]:] = 0"""
    dev = yseg.device
    pred = _new(plan.B, plan.L, dev=dev)
    if plan.uniform:
        _run("k_tola", 0.0, K._lib().se_train_ola_fwd, sig, _p(yseg), _p(pred), plan.B, plan.L, plan.skip, K._st())
    else:
        _run("k_tola", 0.0, K._lib().se_train_ola_fwd_rows, sig, _p(yseg), _p(pred), plan.B, plan.L, _ip(row_table(plan, dev, "skip")), _ip(row_table(plan, dev, "len")), K._st())
    return pred


def synthesis(plan, sig, Y):
    """Y [S][T][F0][2] -> pred [B][L]: iSTFT of every segment, then overlap-add"""
    yseg = _new(Y.shape[0], plan.Ks, dev=Y.device)
    istft(sig, Y, yseg)
    return overlap_add(plan, sig, yseg)


def synthesis_adjoint(plan, sig, dpred):
    """dpred [B][L] -> dY [S][T][F0][2]: the adjoint of overlap-add (dpred[b][lengths[b]:] is never read), then of the iSTFT (an STFT
    of every segment)"""
    B, N, dev = plan.B, plan.N, dpred.device
    gseg = _new(N * B, plan.Ks, dev=dev)
    if plan.uniform:
        _run("k_tola", 0.0, K._lib().se_train_ola_bwd, sig, _p(dpred), _p(gseg), B, N, plan.L, plan.skip, K._st())
    else:
        _run("k_tola", 0.0, K._lib().se_train_ola_bwd_rows, sig, _p(dpred), _p(gseg), B, N, plan.L, _ip(row_table(plan, dev, "skip")), _ip(row_table(plan, dev, "len")), K._st())
    return _stft(sig, gseg, N * B, 1, plan.Ks, 0, 0, 1, plan.T, plan.F0).view(N * B, plan.T, plan.F0, 2)


def gru_steps(plan, dev, T, per, n0=0, Nc=None):
    """Step counts of a GRU launch over segments [n0, n0 + Nc) with `per` streams per utterance, stream-major: live segments x T, a
    device int32 [B * per] - and the live counts, a device int64 [B] for own_last_slab.  Uniform: (None, None), every stream runs all."""
    if plan.uniform:
        return None, None
    live = plan.live(n0, Nc)
    return torch.tensor(live, dtype=torch.int32).mul_(T).repeat_interleave(per).to(dev, non_blocking=True), _rows(live, dev)


def gru_steps_bwd(plan, dev, T, per):
    """Step counts of the backward sweep, one sequence per (stream, segment): T where the segment is the utterance's own, else 0 - a
    device int32 [B * per * N]; None when uniform."""
    if plan.uniform:
        return None
    steps = (torch.arange(plan.N)[None, :] < torch.tensor(plan.Nb)[:, None]).to(torch.int32).mul_(T).repeat_interleave(per, dim=0)
    return steps.reshape(-1).to(dev, non_blocking=True)


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
