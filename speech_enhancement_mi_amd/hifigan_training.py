"""HiFi-GAN generator training on the kernels: `HifiFunction`, the ONE autograd node behind `Generator.realtime_process` of a GPU tensor
with grad enabled after `use_hip_training(True)` (reference training step: Hifi_GAN.train_stage, hifigan.py:917-937).

Forward: the inference kernel path as it stands (`Generator._kernel_process`: the same launches, so both outputs and the carried state
are bit-equal to an eval-mode call and either kind of call continues the other), recording per pass the state the pass entered with.
Nothing else is kept: the fused postnet keeps no activations.

Backward: the overlap-add / iSTFT adjoint of both cotangents once for the call, then pass by pass - the passes are independent given
their entry state, because the reference detaches everything that crosses a window seam (conv history, (h, c), running mean): re-run
the pass up to the decoder's output with its activations kept (`_kernel_pass(..., sv)`), re-run the postnet layer by layer keeping the
twelve pre-activations (the memory rule: 12 x Nc B x 128 x T x F floats, one pass at a time, bounded by max_segments), then
  masks (se_train_mask_bwd) -> postnet (se_hifi_gate_bwd, 1x1 data gradients on se_train_conv_w, weight gradients on the
  deterministic wgrad) -> decoder (se_hifi_skip_bwd / gate_bwd, the transposed convolutions' adjoints) -> norm + tanh
  (se_hifi_seqnorm_bwd) -> fc -> LSTM layers (se_hifi_lstm_bwd: one launch per step for ALL windows of the pass, then GEMMs for
  dW_ih, dW_hh, dx) -> se_hifi_rows_bwd -> encoder.
The kernels give the gradient of the FOLDED weights; per-pass gradients are summed in pass order, and (weight_g, weight_v) receive
theirs on the host through the differentiable fold `hifigan._w`.  No float atomics anywhere: two runs give bit-equal gradients.
`deconvlist[-1].residual*` are unused by the forward and get None, the mixture gets None.

Chunk chains (`use_hip_training(True, chains=True)`): the forward is `_kernel_process` on the chains plan - the sorted-prefix schedule of
the inference path, bit for bit - and records each pass's mixture rows as well.  The backward permutes both cotangents into the
scheduler's sorted order, takes their synthesis adjoint on the sorted plan (nothing beyond a stream's length is read, and the windows
past a stream's own are exact zeros), and differentiates pass by pass on the pass's Bp leading streams.  DEAD WINDOWS - windows of a
pass past a stream's own last one - are run, as the inference path runs them, and carry a ZERO cotangent through the convolution
stack: every activation there is finite, so they add exact zeros to the fixed-order sums.  The kernels whose result depends on a
stream's own schedule take their `_rows` form: se_hifi_lstm_train_fwd_rows (zeros as a finished step's gates and cell),
se_hifi_seqnorm_bwd_rows (per-stream step, zeros at dead windows), se_hifi_lstm_bwd_rows (dead rows not swept, zero dgates).  A
uniform call on one step count runs exactly the launches it ran before."""
from __future__ import annotations

import torch

from . import train_ops as K
from .hifigan import POST_LAYERS, _w
from .train_stages import (_ip, _new, _p, _rows, _run, colsum3, colsum_tall, conv_w, gemm_tn, grads_in_parameter_order, synthesis_adjoint, transpose, wgrad)


def _gate(x):
    y = torch.empty_like(x)
    _run("k_hifi_gate", 0.0, K._lib().se_hifi_gate, _p(x), _p(y), x.numel(), K._st())
    return y


def _gate_bwd(dy, x):
    dx = torch.empty_like(x)
    _run("k_hifi_gate_bwd", 0.0, K._lib().se_hifi_gate_bwd, _p(dy), _p(x), _p(dx), x.numel(), K._st())
    return dx


def _bias_grad(dy, S, Cc):
    """dy [S][Cc][T][F] -> [Cc]: per-(stream, channel) sums, then the fixed-order fold over the streams"""
    part = _new(S, Cc, dev=dy.device)
    _run("k_hifi_chansum", 0.0, K._lib().se_hifi_chansum, _p(dy), _p(part), S * Cc, dy.numel() // (S * Cc), K._st())
    return colsum3(S, (part, Cc))[0]


def _add(dst, src):
    _run("k_tadd", 0.0, K._lib().se_train_add, _p(dst), _p(src), dst.numel(), K._st())


def _postnet_bwd(model, hdec, spec, dY, grads, zero_bias, S, M, T, F0, n_fft):
    """The postnet and the final mask of one pass, re-run layer by layer and differentiated.  hdec [S][2][T][F0] the decoder's output,
    dY the (raw STFT) cotangent of the masked spectrum after the postnet -> the gradient that reaches hdec through the postnet"""
    lib, dev = K._lib(), hdec.device
    ws = [model._folded(("post", l), blk.conv).view(blk.conv.weight_v.shape[0], blk.conv.weight_v.shape[1]) for l, blk in enumerate(model.postnet)]
    pre, a = [], hdec
    for l, blk in enumerate(model.postnet):
        Co, Ci = ws[l].shape
        y = _new(S, Co, T, F0, dev=dev)
        conv_w(3, _p(a), None, ws[l], Ci, 1, blk.conv.bias, y, S, Ci, Co, T, F0, F0, 0)
        pre.append(y)
        a = _gate(y)
    da = torch.empty_like(a)
    _run("k_tmask", 0.0, lib.se_train_mask_bwd, _p(dY), _p(a), _p(spec), _p(da), S, M, T, F0, n_fft, K._st())
    for l in range(POST_LAYERS - 1, -1, -1):
        Co, Ci = ws[l].shape
        name = f"postnet.{l}.conv."
        dy = _gate_bwd(da, pre[l])
        a = hdec if l == 0 else _gate(pre[l - 1])
        pre[l] = None
        grads[name + "bias"] = _bias_grad(dy, S, Co)
        grads[name + "weight"] = wgrad(dy, a, None, S, Co, Ci, T, F0, F0, 0, 1)
        da = _new(S, Ci, T, F0, dev=dev)
        conv_w(3, _p(dy), None, ws[l], 1, Ci, zero_bias, da, S, Co, Ci, T, F0, F0, 0)
    return da


def _pass_backward(model, mixture, rec, dY, dYb, grads):
    """One pass of the call: re-run with the activations kept, then every gradient of the pass into `grads` (names of the folded
    weights end in `.weight`).  dY / dYb [Nc B][T][F0][2]: the cotangents of the pass's masked spectra, after / before the postnet.
    mixture: the pass's rows.  Where the re-run took the norm's `_rows` form (a chains plan, or entry step counts that differ), the
    norm and the LSTM backward take theirs; a uniform pass takes the scalar kernels, as it always has."""
    plan, sig, entry, n0, Nc, start = rec[:6]
    lib, st, dev = K._lib(), K._st, mixture.device
    c = model._cfg
    B, M, T, F0, ch, Fq, H, NL, Lv = plan.B, mixture.shape[1], plan.T, plan.F0, plan.ch, plan.Fq, c["hidden"], c["num_layers"], len(model.convlist)
    S, TT, n_fft = Nc * B, Nc * T, c["n_fft"]
    sv = {}
    state = {k: list(v) if isinstance(v, list) else v for k, v in entry.items()}
    model._kernel_pass(mixture, plan, sig, state, n0, Nc, None, start, sv)
    del state
    zero_bias = torch.zeros(256, device=dev)
    spec, xin, hdec = sv["spec"], sv["xin"], sv["hdec"]
    # both masks and the postnet -> the gradient of the decoder's output
    dout = torch.empty_like(hdec)
    _run("k_tmask", 0.0, lib.se_train_mask_bwd, _p(dYb), _p(hdec), _p(spec), _p(dout), S, M, T, F0, n_fft, st())
    _add(dout, _postnet_bwd(model, hdec, spec, dY, grads, zero_bias, S, M, T, F0, n_fft))
    del hdec
    # decoder, last level first
    dres = {}
    for j in range(Lv - 1, -1, -1):
        blk, r = model.deconvlist[j], sv["dec"][j]
        Ci, Co, Fi, Fy = r["Ci"], r["Co"], r["Fi"], r["Fy"]
        name = f"deconvlist.{j}."
        if j < Lv - 1:
            k, Cr, Fr = r["k"], r["Cr"], r["Fr"]
            duv, dyd = _new(S, 2 * Co, T, Fr, dev=dev), _new(S, Co, T, Fy, dev=dev)
            _run("k_hifi_skip_bwd", 0.0, lib.se_hifi_skip_bwd, _p(dout), _p(r["yd"]), _p(r["uv"]), _p(duv), _p(dyd), S, Co, T, Fy, Fr, st())
            dbuv = _bias_grad(duv, S, 2 * Co)
            grads[name + "residual.bias"], grads[name + "residualmask.bias"] = dbuv[:Co], dbuv[Co:]
            dwuv = wgrad(duv, _p(xin[k], B * Cr * T * Fr), None, S, 2 * Co, Cr, T, Fr, Fr, 0, 1).view(2 * Co, Cr)
            grads[name + "residual.weight"], grads[name + "residualmask.weight"] = dwuv[:Co], dwuv[Co:]
            wuv = torch.cat([model._folded(("res", j), blk.residual).view(Co, Cr), model._folded(("resmask", j), blk.residualmask).view(Co, Cr)])
            dres[k] = _new(S, Cr, T, Fr, dev=dev)
            conv_w(3, _p(duv), None, wuv, 1, Cr, zero_bias, dres[k], S, 2 * Co, Cr, T, Fr, Fr, 0)
            del duv
        else:
            dyd = _gate_bwd(dout, r["yd"])
        grads[name + "conv.bias"] = _bias_grad(dyd, S, Co)
        grads[name + "conv.weight"] = wgrad(r["x_in"], dyd, None, S, Ci, Co, T, Fi, Fy, 2 ** j, 15)
        dout = _new(S, Ci, T, Fi, dev=dev)
        conv_w(0, _p(dyd), None, model._folded(("deconv", j), blk.conv), Co * 15, 15, zero_bias, dout, S, Co, Ci, T, Fy, Fi, 2 ** j)
        del dyd
    sv["dec"] = None
    # bottleneck: running-mean norm + tanh, fc, the LSTM layers in reverse
    Cl, Fl = ch[Lv], Fq[Lv]
    D = Cl * Fl
    nm, fc, m = model.gru.norm, model.gru.fc_output_layer, model.gru.sequence_model
    do, em = _new(B * TT, D, dev=dev), _new(S, dev=dev)
    pw, pb = _new(S, D, dev=dev), _new(S, D, dev=dev)
    rows = sv["rows"]
    if rows:   # dead windows: zeros to their rows of `do` and to their slabs, dout unread there
        _run("k_hifi_seqnorm_bwd", 0.0, lib.se_hifi_seqnorm_bwd_rows, _p(dout), _p(sv["o"]), _p(nm.weight), _p(sv["wm"]), _ip(sv["step_rows"]), _ip(sv["cnt"]),
             _p(em), _p(do), _p(pw), _p(pb), Nc, B, Cl, T, Fl, st())
        live = torch.tensor(plan.live(n0, Nc), dtype=torch.int32).to(dev, non_blocking=True)
    else:
        _run("k_hifi_seqnorm_bwd", 0.0, lib.se_hifi_seqnorm_bwd, _p(dout), _p(sv["o"]), _p(nm.weight), _p(sv["wm"]), sv["step"], _p(em), _p(do), _p(pw), _p(pb),
             Nc, B, Cl, T, Fl, st())
    grads["gru.norm.weight"], grads["gru.norm.bias"] = colsum3(S, (pw, D), (pb, D))
    del dout, pw, pb
    wfc = model._folded("fc", fc)
    grads["gru.fc_output_layer.weight"] = gemm_tn(do, sv["lstm"][NL - 1]["out"])
    grads["gru.fc_output_layer.bias"] = colsum_tall(do)
    dlayer = K._gemm(do, transpose(wfc))
    del do
    for l in range(NL - 1, -1, -1):
        r = sv["lstm"][l]
        w_ih, w_hh = getattr(m, f"weight_ih_l{l}"), getattr(m, f"weight_hh_l{l}")
        dg, dc, whht = _new(B * TT, 4 * H, dev=dev), _new(B * Nc, H, dev=dev), transpose(w_hh.detach())
        hp, cp = _new(B * TT, H, dev=dev), _new(B * TT, H, dev=dev)   # h_{t-1}, c_{t-1} of every row: shifted by one step, the pass's entry state in front
        _run("k_gru_hprev", 0.0, lib.se_train_gru_hprev, _p(r["out"]), _p(r["h0"]), _p(hp), B, TT, H, TT, 0, TT, st())
        _run("k_gru_hprev", 0.0, lib.se_train_gru_hprev, _p(r["cs"]), _p(r["c0"]), _p(cp), B, TT, H, TT, 0, TT, st())
        if rows:   # only a stream's own windows are swept; the dgates of the others are exact zeros
            _run("k_hifi_lstm_bwd_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm_bwd_rows, _p(dlayer), _p(r["gates"]), _p(r["cs"]), _p(cp), _p(whht), _p(dg),
                 _p(dc), _ip(live), B, Nc, T, H, st())
        else:
            _run("k_hifi_lstm_bwd_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm_bwd, _p(dlayer), _p(r["gates"]), _p(r["cs"]), _p(cp), _p(whht), _p(dg), _p(dc),
                 B, Nc, T, H, st())
        pre = "gru.sequence_model."
        grads[pre + f"weight_ih_l{l}"] = gemm_tn(dg, sv["xs"][l])
        grads[pre + f"weight_hh_l{l}"] = gemm_tn(dg, hp)
        grads[pre + f"bias_ih_l{l}"] = grads[pre + f"bias_hh_l{l}"] = colsum_tall(dg)
        dlayer = K._gemm(dg, transpose(w_ih.detach()))
        sv["lstm"][l] = None
        del dg, hp, cp
    dgated = _new(S, Cl, T, Fl, dev=dev)
    _run("k_hifi_rows_bwd", 0.0, lib.se_hifi_rows_bwd, _p(dlayer), _p(dgated), Nc, B, Cl, T, Fl, st())
    del dlayer
    # encoder, last level first: the features carry no gradient, and nothing flows into a window's time history (detached)
    for i in range(Lv - 1, -1, -1):
        blk = model.convlist[i]
        Ci, Co, Fi, Fo, d = ch[i], ch[i + 1], Fq[i], Fq[i + 1], 2 ** i
        name = f"convlist.{i}."
        dy = _gate_bwd(dgated, sv["ypre"][i])
        sv["ypre"][i] = None
        grads[name + "conv.bias"] = _bias_grad(dy, S, Co)
        grads[name + "conv.weight"] = wgrad(dy, _p(xin[i], B * Ci * T * Fi), _p(xin[i]), S, Co, Ci, T, Fo, Fi, d, 15)
        if i == 0:
            break
        dgated = _new(S, Ci, T, Fi, dev=dev)
        w = model._folded(("conv", i), blk.conv)
        for kind in (1, 2):
            conv_w(kind, _p(dy), None, w, 15, Ci * 15, zero_bias, dgated, S, Co, Ci, T, Fo, Fi, d)
        _add(dgated, dres.pop(i))
        del dy


def _normed_modules(model):
    Lv = len(model.convlist)
    mods = [(f"convlist.{i}.conv", b.conv) for i, b in enumerate(model.convlist)] + [(f"deconvlist.{j}.conv", b.conv) for j, b in enumerate(model.deconvlist)]
    for j, b in enumerate(model.deconvlist[:Lv - 1]):
        mods += [(f"deconvlist.{j}.residual", b.residual), (f"deconvlist.{j}.residualmask", b.residualmask)]
    return mods + [("gru.fc_output_layer", model.gru.fc_output_layer)] + [(f"postnet.{l}.conv", b.conv) for l, b in enumerate(model.postnet)]


class HifiFunction(torch.autograd.Function):
    """(pred, pred_before) = Generator.realtime_process(mixture, post=True, reset) on the kernels, forward AND backward, as one autograd
    node.  forward(ctx, model, mixture, plan, *params), params in named_parameters() order; plan: the call's CallPlan, uniform or
    (use_hip_training(True, chains=True)) chains."""

    @staticmethod
    def forward(ctx, model, mixture, plan, *params):
        mix = mixture.detach().contiguous().float()
        record = []
        pred, before = model._kernel_process(mix, plan, record)
        ctx.model, ctx.mix, ctx.plan, ctx.record = model, mix, plan, record
        return pred, before

    @staticmethod
    def backward(ctx, dpred, dbefore):
        model, mix, plan, record = ctx.model, ctx.mix, ctx.plan, ctx.record
        B = plan.B
        # the first pass runs every stream, so its plan is the call's as the passes see it: the caller's when uniform, else the
        # scheduler's sorted one, whose `rows` are the caller's rows in sorted order
        sp, sig = record[0][0], record[0][1]
        order = None if plan.uniform else _rows(sp.rows, mix.device)
        zeros = None
        cots = []
        for d in (dpred, dbefore):
            if d is None:
                d = zeros = torch.zeros(B, plan.L, device=mix.device) if zeros is None else zeros
            d = d.contiguous().float()
            cots.append(synthesis_adjoint(sp, sig, d if order is None else d.index_select(0, order)))   # [N B][T][F0][2], window-major
        total = {}
        with torch.no_grad():
            for rec in record:   # in pass order: the sums below have one fixed order
                n0, Nc, Bp = rec[3], rec[4], rec[0].B
                grads = {}
                if Bp == B:
                    dY, dYb = (c[n0 * B:(n0 + Nc) * B] for c in cots)
                else:   # a prefix pass: its Bp leading streams of every window
                    dY, dYb = (c.view(sp.N, B, *c.shape[1:])[n0:n0 + Nc, :Bp].reshape(Nc * Bp, *c.shape[1:]) for c in cots)
                _pass_backward(model, rec[6], rec, dY, dYb, grads)
                for k, g in grads.items():
                    total[k] = g if k not in total else total[k] + g
        out = {}
        for name, m in _normed_modules(model):   # folded weight -> (weight_g, weight_v), through the differentiable fold
            dW = total.pop(name + ".weight")
            with torch.enable_grad():
                w = _w(m)
                out[name + ".weight_g"], out[name + ".weight_v"] = torch.autograd.grad(w, [m.weight_g, m.weight_v], dW.reshape(w.shape))
        out.update(total)
        ctx.record = ctx.mix = None
        return (None, None, None, *grads_in_parameter_order(model, out))
