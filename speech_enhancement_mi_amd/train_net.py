"""The whole differentiable `realtime_process` of TemporalCRN (CRN.py:560-589 over 454-496) on hand-written kernels, forward
AND backward, as ONE torch.autograd.Function (reference training step train.py:195-204).

Every stage is a `se_train_*` / `se_sig_*` launch (csrc/train_fused.hip.h, gru_pseq.hip.h, train_ops.inc.h), torch glue included;
PyTorch only allocates tensors, and autograd sees a single node whose backward returns the parameter gradients.  No float
atomics: gradients are bit-reproducible.

This module is CRNFunction only, orchestration over named stages (`_pre_*`: features + pre-conv chain, `_encoder_*`, `_gru_*`: GRU +
fc, then decoder, mask and signal chain).  What general_beamformer.py and fsn_training.py share with it - launch helpers (still
importable from here), geometry, signal chain, plain encoder block, decoder, GRU layer backward - lives in train_stages.py.

Layout: S = N segments x B utterances, SEGMENT-major.  An encoder block's time history (the reference's `buffer`,
CRN.py:325-337 = the previous segment's detached input) is then the same tensor one slab of B streams earlier, so each layer
runs once over all S streams with `xprev = x - one slab`; slab 0 of every input tensor holds the carried state (zeros after a
reset).  The GRU runs once per layer over the N*T steps of every utterance (one persistent launch), with the BPTT cut at
segment seams exactly where the reference detaches `h` (CRN.py:281).
"""
from __future__ import annotations

import torch

from . import train_ops as K
from .train_stages import (_cs, _new, _p, _run, _sig, colsum3, colsum_tall, conv_w, decoder_bwd, decoder_fwd,
                           encoder_block_bwd, encoder_block_fwd, encoder_conv_bwd, gemm_tn, gln_bwd, gln_fwd, grads_in_parameter_order,
                           gru_layer_bwd, input_features, own_last_slab, row_table, slab_gather, start_rows, stft, synthesis, synthesis_adjoint,
                           transpose, wgrad, call_plan)

_side_streams = {}
PIPELINE_LAYERS = True   # training forward: GRU layers as a wavefront over segments on one HIP stream per layer (False: layer after layer)


def _side_stream(dev, idx):
    key = (dev.index, idx)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams[key]


def _first_slab(t, state, key, idx, q):   # slab 0 = the carried state of a flag=True continuation, zeros after a reset
    if state is None or state.get(key) is None:
        t[0].zero_()
    else:   # ... chunk chains: per utterance
        start_rows(q["plan"], state[key][idx], dst=t[0])


def _inject(dpre, gf, S, Cc, X):   # dpre += d feature map; -> the bias gradient (per-channel sums of the result)
    part = _new(S, Cc, dev=dpre.device)
    _run("k_add_csum", 0.0, K._lib().se_train_add_csum, _p(dpre), _p(gf), _p(part), S, Cc, X, K._st())
    return colsum3(S, (part, Cc))[0]


def gate_pair(a_t, blk, y_ptr, ys, S, Co, T, Fo, em):
    """CRN_ELU.py:240-241: conv_trans(a) * sigmoid(conv_gated(a)) -> gLN.  Two 1x1 launches into the halves of tg."""
    dev = a_t.device
    tg = _new(S, 2 * Co, T, Fo, dev=dev)
    conv_w(3, _p(a_t), None, blk.conv_trans.weight, Co, 1, blk.conv_trans.bias, tg, S, Co, Co, T, Fo, Fo, 0, 0, 2 * Co, 0)
    conv_w(3, _p(a_t), None, blk.conv_gated.weight, Co, 1, blk.conv_gated.bias, tg, S, Co, Co, T, Fo, Fo, 0, 0, 2 * Co, Co)
    stt = _new(S, 2, dev=dev)
    _run("k_tgate_fwd", 0.0, K._lib().se_train_gate_fwd, _p(tg), _p(blk.norm.weight), _p(blk.norm.bias), y_ptr, *ys, _p(stt), S, Co, T, Fo, em, K._st())
    return tg, stt


def gate_pair_bwd(dy_ptr, ds, a_t, tg, stt, blk, pre, grads, zero_bias, S, Co, T, Fo, em):
    """through gLN + gated pair + ELU: returns dy of the convolution that produced a_t (in place in a fresh tensor)."""
    lib = K._lib()
    dev = a_t.device
    dtg = _new(S, 2 * Co, T, Fo, dev=dev)
    pw, pb, pbias = _new(S, Co, dev=dev), _new(S, Co, dev=dev), _new(S, 2 * Co, dev=dev)
    _run("k_tgate_bwd", 0.0, lib.se_train_gate_bwd, dy_ptr, *ds, _p(tg), _p(blk.norm.weight), _p(stt), _p(dtg), _p(pw), _p(pb), _p(pbias), S, Co, T, Fo, em, K._st())
    dnw, dnb, dbtg = colsum3(S, (pw, Co), (pb, Co), (pbias, 2 * Co))
    grads[pre + "norm.weight"], grads[pre + "norm.bias"] = dnw, dnb
    grads[pre + "conv_trans.bias"], grads[pre + "conv_gated.bias"] = dbtg[:Co], dbtg[Co:]
    dwtg = wgrad(dtg, a_t, None, S, 2 * Co, Co, T, Fo, Fo, 0, 1).view(2 * Co, Co)
    grads[pre + "conv_trans.weight"], grads[pre + "conv_gated.weight"] = dwtg[:Co], dwtg[Co:]
    wst = _new(2 * Co, Co, dev=dev)   # [conv_trans; conv_gated] stacked: d a = W^T dtg in one 2Co-deep contraction
    wst[:Co].copy_(blk.conv_trans.weight.view(Co, Co)); wst[Co:].copy_(blk.conv_gated.weight.view(Co, Co))
    da = _new(S, Co, T, Fo, dev=dev)
    conv_w(3, _p(dtg), None, wst, 1, Co, zero_bias, da, S, 2 * Co, Co, T, Fo, Fo, 0)
    pp = _new(S, Co, dev=dev)
    _run("k_telu_bwd", 0.0, lib.se_train_elu_bwd, _p(da), _p(a_t), _p(pp), S, Co, T, Fo, K._st())
    grads[pre + "conv.bias"] = colsum3(S, (pp, Co))[0]
    return da


# ---- the stages of CRNFunction: q = the call's dimensions, sv = what the forward saves for the backward ---------------------------
def _plan(model, mixture, flag=False, lengths=None, uniform=None):
    """the CallPlan of realtime_process(mixture, flag, lengths) on this model: the U-Net level sizes come with it.  uniform=False: the
    chains form (the `_rows` kernels) whatever the triage says"""
    B, M, L = mixture.shape
    ch = [2 * M - 1] + [blk.conv.weight.shape[0] for blk in model.convlist]
    return call_plan(flag, lengths, B, L, model.segment_length, model._hop, model._cfg_args["n_fft"], ch, uniform)


def _dims(model, mixture, plan):
    """q = the plan's geometry and the model's own sizes"""
    B, M, L = mixture.shape
    if plan.B != B or plan.L != L:
        raise ValueError(f"the call plan describes a batch of {plan.B} utterances of up to {plan.L} samples, not {B} of {L}")
    g = model.gru.sequence_model
    Lv = len(model.convlist)
    CL, FL = plan.ch[Lv], plan.Fq[Lv]
    n_fft = model._cfg_args["n_fft"]
    q = dict(plan.geo, plan=plan, L=L, B=B, M=M, S=plan.N * B, Lv=Lv, H=g.hidden_size, NL=g.num_layers, CL=CL, FL=FL, D=CL * FL, n_fft=n_fft,
             sig=_sig(mixture.device, n_fft, model._win, model._hop, model.segment_length))
    return q


def _pre_fwd(model, q, sv, state):
    """spec -> features and, variants 1 / 2, x = block(x) + x three times (CRN_ELU.py:375-376) -> [N + 1][B][C0][T][F0]"""
    lib = K._lib()
    N, B, S, M, T, F0, C0 = q["N"], q["B"], q["S"], q["M"], q["T"], q["F0"], q["ch"][0]
    V, dev = sv["V"], sv["spec"].device
    cur = _new(N + 1, B, C0, T, F0, dev=dev)
    slab0 = B * C0 * T * F0
    _first_slab(cur, state, "pbuf" if V else "buf", 0, q)
    input_features(sv["spec"], cur, S, B, M, C0, T, F0, 1 if V == 1 else 0)
    sv["pre"] = []
    if V:
        for k, blk in enumerate(model.preconvlist):
            a_t = _new(S, C0, T, F0, dev=dev)
            _run("k_pre5", 2.0 * S * C0 * C0 * 25 * T * F0, lib.se_train_pre5, 0, _p(cur, slab0), _p(cur), _p(blk.conv.weight), _p(blk.conv.bias), None, _p(a_t),
                 S, C0, T, F0, 2 ** k, 2, K._st())
            out = _new(S, C0, T, F0, dev=dev)
            tg, stt = gate_pair(a_t, blk, _p(out), _cs(C0, T, F0), S, C0, T, F0, sv["em"])
            nxt = _new(N + 1, B, C0, T, F0, dev=dev)
            _first_slab(nxt, state, "pbuf", k + 1, q) if k < 2 else _first_slab(nxt, state, "buf", 0, q)
            _run("k_tadd", 0.0, lib.se_train_add3, _p(nxt, slab0), _p(out), _p(cur, slab0), S * C0 * T * F0, K._st())
            sv["pre"].append(dict(cur=cur, a=a_t, tg=tg, st=stt))
            cur = nxt
    return cur


def _pre_bwd(model, q, sv, dnxt, grads, zero_bias):
    """the pre-conv chain, last block first: x_{k+1} = block_k(x_k) + x_k"""
    lib = K._lib()
    B, S, T, F0, C0 = q["B"], q["S"], q["T"], q["F0"], q["ch"][0]
    slab0 = B * C0 * T * F0
    for k in range(2, -1, -1):
        blk, r = model.preconvlist[k], sv["pre"][k]
        pre = f"preconvlist.{k}."
        dyk = gate_pair_bwd(_p(dnxt), _cs(C0, T, F0), r["a"], r["tg"], r["st"], blk, pre, grads, zero_bias, S, C0, T, F0, sv["em"])
        part = _new(S, C0 * C0 * 25, dev=dyk.device)
        _run("k_pre5", 2.0 * S * C0 * C0 * 25 * T * F0, lib.se_train_pre5, 2, _p(r["cur"], slab0), _p(r["cur"]), _p(blk.conv.weight), None, _p(dyk), _p(part),
             S, C0, T, F0, 2 ** k, 0, K._st())
        grads[pre + "conv.weight"] = colsum3(S, (part, C0 * C0 * 25))[0]
        if k == 0:
            break  # block 0 reads the features
        dcur = _new(S, C0, T, F0, dev=dyk.device)
        _run("k_pre5", 2.0 * S * C0 * C0 * 25 * T * F0, lib.se_train_pre5, 1, None, None, _p(blk.conv.weight), None, _p(dyk), _p(dcur), S, C0, T, F0, 2 ** k, 0, K._st())
        _run("k_tadd", 0.0, lib.se_train_add, _p(dcur), _p(dnxt), dcur.numel(), K._st())
        dnxt = dcur


def _encoder_fwd(model, q, sv, state, x_full, features):
    """The last block writes the GRU layout [S][T][D], feature index c * F + f (CRN.py:476-478).  -> f0 (features only)"""
    N, B, S, T, Lv, ch, Fq = q["N"], q["B"], q["S"], q["T"], q["Lv"], q["ch"], q["Fq"]
    V, em, dev = sv["V"], sv["em"], x_full.device
    xin, ys, stats_e, enc_tg, f0 = [x_full], [], [], [], None
    for i, blk in enumerate(model.convlist):
        Ci, Co, Fi, Fo, d = ch[i], ch[i + 1], Fq[i], Fq[i + 1], 2 ** i
        if i < Lv - 1:
            nxt = _new(N + 1, B, Co, T, Fo, dev=dev)
            _first_slab(nxt, state, "buf", i + 1, q)
            y_ptr, ysd = _p(nxt, B * Co * T * Fo), _cs(Co, T, Fo)
            xin.append(nxt)
        else:
            sv["seq"] = _new(S * T, Co * Fo, dev=dev)
            y_ptr, ysd = _p(sv["seq"]), (T * Co * Fo, Fo, Co * Fo)
        if not V:
            y, stt = encoder_block_fwd(blk, xin[i], y_ptr, ysd, S, B, Ci, Co, T, Fi, Fo, d, em)   # y: the pre-activation
        else:
            slab = B * Ci * T * Fi
            y = _new(S, Co, T, Fo, dev=dev)   # ELU(conv), all the backward needs
            conv_w(0, _p(xin[i], slab), _p(xin[i]), blk.conv.weight, Ci * 15, 15, blk.conv.bias, y, S, Ci, Co, T, Fi, Fo, d, 2)
            if features and i == Lv - 1:  # f0: the same convolution without activation
                f0 = _new(S, Co, T, Fo, dev=dev)
                conv_w(0, _p(xin[i], slab), _p(xin[i]), blk.conv.weight, Ci * 15, 15, blk.conv.bias, f0, S, Ci, Co, T, Fi, Fo, d, 0)
            tg, stt = gate_pair(y, blk, y_ptr, ysd, S, Co, T, Fo, em)
            enc_tg.append(tg)
        ys.append(y)
        stats_e.append(stt)
    sv.update(xin=xin, ys=ys, stats_e=stats_e, enc_tg=enc_tg)
    return f0


def _encoder_bwd(model, q, sv, dseq, dres, df0, grads, zero_bias):
    """encoder, last block first; dseq = d seq [S][T][D].  -> the gradient of the first block's input (variants 1 / 2)"""
    B, S, T, Lv, ch, Fq, D, FL = q["B"], q["S"], q["T"], q["Lv"], q["ch"], q["Fq"], q["D"], q["FL"]
    V, em = sv["V"], sv["em"]
    dy_ptr, ds = _p(dseq), (T * D, FL, D)
    dxi = dseq
    for i in range(Lv - 1, -1, -1):
        blk = model.convlist[i]
        geo = (S, B, ch[i], ch[i + 1], T, Fq[i], Fq[i + 1], 2 ** i)
        Co, Fo = ch[i + 1], Fq[i + 1]
        pre = f"convlist.{i}."
        need_dx = bool(i or V)  # variant 0: the features carry no gradient
        if V:
            dy = gate_pair_bwd(dy_ptr, ds, sv["ys"][i], sv["enc_tg"][i], sv["stats_e"][i], blk, pre, grads, zero_bias, S, Co, T, Fo, em)
            if i == Lv - 1 and df0 is not None:
                grads[pre + "conv.bias"] = _inject(dy, df0, S, Co, T * Fo)
            dxi = encoder_conv_bwd(blk, pre, grads, dy, sv["xin"][i], dres.get(i), zero_bias, *geo, need_dx)
        else:
            dxi = encoder_block_bwd(blk, pre, grads, dy_ptr, ds, sv["ys"][i], sv["stats_e"][i], sv["xin"][i], dres.get(i), zero_bias, *geo, em, need_dx)
        if need_dx:
            dy_ptr, ds = _p(dxi), _cs(ch[i], T, Fq[i])
    return dxi


def _gru_fwd(model, q, sv, state):
    """The GRU layers over the N*T steps of every utterance, then the fc layer.  -> (o_fc [S*T][D] pre-activation, final states)"""
    N, B, S, T, H, NL = q["N"], q["B"], q["S"], q["T"], q["H"], q["NL"]
    seq = sv["seq"]
    dev = seq.device
    g = model.gru.sequence_model
    R = S * T
    outs, gates, h0s, hTs = [], [], [], []
    gi0 = K._gemm(seq, g.weight_ih_l0, g.bias_ih_l0)
    for l in range(NL):
        if state is None or state["h"] is None:
            h0s.append(torch.zeros(B, H, device=dev))
        else:
            h0s.append(start_rows(q["plan"], state["h"][l]))
        outs.append(_new(R, H, dev=dev)); gates.append(_new(R, 4 * H, dev=dev))
    if NL == 1 or N < 4 or not PIPELINE_LAYERS or not K._lib().se_train_gru_pseq_supported(B, H):
        layer_in = seq
        for l in range(NL):
            gi = gi0 if l == 0 else K._gemm(layer_in, getattr(g, f"weight_ih_l{l}"), getattr(g, f"bias_ih_l{l}"))
            hT = _new(B, H, dev=dev)
            K._gru_seq_fwd(gi, h0s[l], getattr(g, f"weight_hh_l{l}"), getattr(g, f"bias_hh_l{l}"), outs[l], gates[l], hT, B, N * T, H, T, B * T, T)
            hTs.append(hT)
            layer_in = outs[l]
    else:
        # Layer wavefront over segments: the recurrence is sequential in time, but layer l of segment n only needs layer l - 1 of the
        # SAME segment.  Every layer gets its own HIP stream and walks the utterance one segment (T steps, one persistent launch)
        # at a time; layer l's segment n waits for an event of layer l - 1's segment n, so the layers run one segment apart:
        # (N + NL - 1) x T dependent steps instead of NL x N x T.
        cur = torch.cuda.current_stream()
        streams = [cur] + [_side_stream(dev, l) for l in range(1, NL)]
        hall = [_new(N, B, H, dev=dev) for _ in range(NL)]            # the state after every segment (the next segment's h0)
        gis = [gi0] + [_new(R, 3 * H, dev=dev) for _ in range(1, NL)]
        fork = torch.cuda.Event()
        fork.record(cur)
        for l in range(1, NL):
            streams[l].wait_event(fork)
        done = [[None] * N for _ in range(NL)]
        rows = B * T
        for n in range(N):
            r0, r1 = n * rows, (n + 1) * rows
            for l in range(NL):
                with torch.cuda.stream(streams[l]):
                    if l > 0:
                        streams[l].wait_event(done[l - 1][n])
                        _run("k_gemm_skinny", 2.0 * rows * 3 * H * H, K._lib().se_train_gemm, _p(outs[l - 1], r0 * H), _p(getattr(g, f"weight_ih_l{l}")),
                             _p(getattr(g, f"bias_ih_l{l}")), _p(gis[l], r0 * 3 * H), rows, 3 * H, H, 0, K._st())
                    K._gru_seq_fwd(gis[l][r0:r1], h0s[l] if n == 0 else hall[l][n - 1], getattr(g, f"weight_hh_l{l}"), getattr(g, f"bias_hh_l{l}"), outs[l][r0:r1],
                                   gates[l][r0:r1], hall[l][n], B, T, H, T, 0, T, tag=l)
                    ev = torch.cuda.Event()
                    ev.record(streams[l])
                    done[l][n] = ev
        for l in range(1, NL):
            cur.wait_event(done[l][N - 1])
        hTs = [hall[l][N - 1] for l in range(NL)]
        layer_in = outs[NL - 1]
    fc = model.gru.fc_output_layer
    sv.update(outs=outs, gates=gates, h0s=h0s)
    return K._gemm(layer_in, fc.weight, fc.bias), hTs


def _gru_bwd(model, q, sv, dxd, df1, grads):
    """bottleneck: gLN(last) + activation + fc, then the GRU layers in reverse.  dxd = the gradient of the decoder input.  -> d seq"""
    B, N, S, T, H, NL, D, CL, FL = q["B"], q["N"], q["S"], q["T"], q["H"], q["NL"], q["D"], q["CL"], q["FL"]
    fc, g = model.gru.fc_output_layer, model.gru.sequence_model
    do_fc, dw, db, dpre = gln_bwd(_p(dxd), _cs(CL, T, FL), sv["o_fc"], (T * D, FL, D), model.gru.norm.weight, sv["st_fc"], S, CL, T, FL, 1, sv["act"], sv["em"])
    if df1 is not None:
        _run("k_tadd", 0.0, K._lib().se_train_add, _p(do_fc), _p(df1), do_fc.numel(), K._st())
        dpre = colsum_tall(do_fc)
    grads["gru.norm.weight"], grads["gru.norm.bias"], grads["gru.fc_output_layer.bias"] = dw, db, dpre
    grads["gru.fc_output_layer.weight"] = gemm_tn(do_fc, sv["outs"][NL - 1])
    dlayer = K._gemm(do_fc, transpose(fc.weight))  # [R, H]
    for l in range(NL - 1, -1, -1):
        x_l = sv["seq"] if l == 0 else sv["outs"][l - 1]
        dlayer = gru_layer_bwd(dlayer, sv["outs"][l], sv["gates"][l], sv["h0s"][l], x_l, getattr(g, f"weight_ih_l{l}"), getattr(g, f"weight_hh_l{l}"),
                               "gru.sequence_model.", l, grads, B, N, T, H, T, B * T, T)
    return dlayer


class CRNFunction(torch.autograd.Function):
    """pred = realtime_process(mixture) for the CRN.py (variant 0), CRN_ELU.py (variant 1, the model train.py:16 trains) and
    distillation_crn.py (variant 2) networks.  forward(ctx, model, mixture, plan, *params), plan = _plan(model, mixture, flag, lengths).
    features=True (CRNFeatFunction, variant 2):
    the five distillation feature maps are extra outputs in the training layout - f0, f2..f4 [S][C][T][F] before activation, f1 the
    fc output [S*T][D] - and the backward adds their gradients (None: skipped) into the pre-activation gradients, bias gradients
    included."""

    @staticmethod
    def forward(ctx, model, mixture, plan, *params, features=False):
        K._need_gpu(mixture, params[0])
        mixture = mixture.contiguous()
        V = model._VARIANT            # 0 = CRN.py (ReLU); 1 = CRN_ELU.py (ELU, gated 1x1 pair per block, three 5x5 pre-conv blocks, atan2 phase)
        if V not in (0, 1, 2):        # 2 = distillation_crn.py: variant 1 with arctan phase and gLN denominator sqrt(var) + EPS
            raise NotImplementedError(f"no training kernels for variant {V}")
        if features and V != 2:
            raise ValueError("feature maps exist for the distillation_crn.py architecture (variant 2) only")
        q = _dims(model, mixture, plan)
        B, M, N, S, T, F0, Lv, CL, FL, D = (q[k] for k in ("B", "M", "N", "S", "T", "F0", "Lv", "CL", "FL", "D"))
        state = model._state if plan.any_flag else None
        if not plan.uniform and state is not None and state["h"][0].shape[0] != B:
            raise RuntimeError(f"flag=True continues row b of the carried state, which holds {state['h'][0].shape[0]} utterances, not {B}")
        act, em = 2 if V else 1, 1 if V == 2 else 0   # em = eps_mode of every gLN
        sv = dict(V=V, act=act, em=em)  # saved for backward
        spec = sv["spec"] = stft(plan, q["sig"], mixture, M)
        f0 = _encoder_fwd(model, q, sv, state, _pre_fwd(model, q, sv, state), features)
        o_fc, hTs = _gru_fwd(model, q, sv, state)
        xd = _new(S, CL, T, FL, dev=spec.device)
        sv["o_fc"] = o_fc
        sv["st_fc"] = gln_fwd(o_fc, (T * D, FL, D), _p(xd), _cs(CL, T, FL), model.gru.norm.weight, model.gru.norm.bias, S, CL, T, FL, FL, 1, act, em)
        xl, dec = sv["xl"], sv["dec"] = decoder_fwd(model.deconvlist, sv["xin"] + [xd], q["ch"], q["Fq"], S, B, T, act, em)
        if xl.shape[1] != 2 or xl.shape[3] != F0:
            raise RuntimeError("last decoder block must produce the 2-channel mask at full resolution")
        Y = _new(S, T, F0, 2, dev=spec.device)
        _run("k_tmask", 0.0, K._lib().se_train_mask_fwd, _p(xl), _p(spec), _p(Y), S, M, T, F0, K._st())
        pred = synthesis(plan, q["sig"], Y)
        # carried state for a flag=True continuation (detached by construction): the block inputs after every utterance's OWN last
        # segment (slab Nb[b]) and the GRU state there - chains: the layer outputs' row of step Nb[b] * T - 1
        H, dev = q["H"], spec.device
        model._state = dict(buf=[own_last_slab(plan, sv["xin"][i]) for i in range(Lv)], pbuf=[own_last_slab(plan, r["cur"]) for r in sv["pre"]] if V else None,
                            h=hTs if plan.uniform else [slab_gather(o, row_table(plan, dev, "lastseg"), B, H, B * T * H, T * H, (T - 1) * H) for o in sv["outs"]])
        ctx.model, ctx.dims, ctx.sv = model, q, sv
        if features:
            return (pred, f0, o_fc) + tuple(r["yd"] for r in dec[:Lv - 1])
        return pred

    @staticmethod
    def backward(ctx, dpred, *dfeats):
        model, q, sv = ctx.model, ctx.dims, ctx.sv
        B, M, N, S, T, F0, Lv = (q[k] for k in ("B", "M", "N", "S", "T", "F0", "Lv"))
        dev = sv["spec"].device
        if dpred is None:  # features=True and only the feature maps reach the loss
            dpred = torch.zeros(B, q["L"], device=dev)
        dpred = dpred.contiguous()
        grads = {}
        dfeats = [None if g is None else g.contiguous() for g in dfeats] + [None] * (2 + Lv - 1 - len(dfeats))
        zero_bias = torch.zeros(256, device=dev)

        def feature_hook(j, dyd, rec):  # variant 2: the gradient of feature map 2 + j enters before the activation of level j
            if j < Lv - 1 and dfeats[2 + j] is not None:
                return _inject(dyd, dfeats[2 + j], S, rec["Co"], T * rec["Fy"])

        dY = synthesis_adjoint(q["plan"], q["sig"], dpred)
        dx = _new(S, 2, T, F0, dev=dev)
        _run("k_tmask", 0.0, K._lib().se_train_mask_bwd, _p(dY), _p(sv["xl"]), _p(sv["spec"]), _p(dx), S, M, T, F0, q["n_fft"], K._st())
        dxd, dres = decoder_bwd(model.deconvlist, sv["dec"], sv["xin"], dx, grads, zero_bias, S, B, T, sv["act"], sv["em"], hook=feature_hook)
        dseq = _gru_bwd(model, q, sv, dxd, dfeats[1], grads)
        dx0 = _encoder_bwd(model, q, sv, dseq, dres, dfeats[0], grads, zero_bias)
        if sv["V"]:
            _pre_bwd(model, q, sv, dx0, grads, zero_bias)
        ctx.sv = None
        return (None, None, None, *grads_in_parameter_order(model, grads))


class CRNFeatFunction(torch.autograd.Function):
    """CRNFunction with features=True: (pred, f0, f1, f2, ...)."""

    @staticmethod
    def forward(ctx, model, mixture, plan, *params):
        ctx.set_materialize_grads(False)
        return CRNFunction.forward(ctx, model, mixture, plan, *params, features=True)

    @staticmethod
    def backward(ctx, dpred, *dfeats):
        return CRNFunction.backward(ctx, dpred, *dfeats)


def realtime_process_fused(model, mixture, flag=False, features=False, lengths=None):
    """flag: a bool, or one value per utterance ([B] tensor / list); lengths: per-utterance lengths <= mixture.shape[-1] (None: all full).
    With either given per utterance, the batch is B independent chunk chains (datagen.ChunkChainBatch): utterance b is zero beyond
    lengths[b] (whatever the padding holds), starts from zero state where flag[b] is False and continues row b of model._state where it is
    True; pred[b, lengths[b]:] = 0 and model._state afterwards holds, per utterance, what that utterance alone would carry.  The feature
    maps of features=True cover all N = max N_b windows of every utterance.  A batch whose flags and lengths are all alike takes the
    scalar kernels, as a bool flag does."""
    params = [p for _, p in model.named_parameters()]
    plan = _plan(model, mixture, flag, lengths)
    if not features:
        return CRNFunction.apply(model, mixture, plan, *params)
    pred, f0, f1, *fd = CRNFeatFunction.apply(model, mixture, plan, *params)
    S, C, T, F = f0.shape
    # the reference layout [N*B, C, F, T] as views: f1 is the fc output [S*T][D] reshaped (not permuted), like distillation_crn.py:368
    return pred, [f0.transpose(2, 3), f1.view(S, C, F, T)] + [f.transpose(2, 3) for f in fd]
