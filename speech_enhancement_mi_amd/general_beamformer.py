"""Drop-in `GeneralBeamformer` (reference GeneralBeamformer.py:266-388, built by train.py / predict.py from config.yaml's
`GeneralBeamformer:` block).

Same constructor, state_dict keys and shapes (the `convlist.i.conv.*` / `net.0.*` aliases and the unused `residual*` modules of the
last decoder block included), same entry points:

    forward(x[B, M, F, T, 2]) -> [B, F, T, 2]          one segment, stateful (GeneralBeamformer.py:318-373)
    realtime_process(mixture[B, M, L], flag, lengths=None) -> [B, L]  GeneralBeamformer.py:449-496; with per-utterance flags /
                                                        lengths the batch is B independent chunk chains (all three paths)
    reset(), compute_loss(source, pred_source, length)

The call's contract, the choice of path, the refusals and the carried state are streaming.StreamingMixin's, shared with gtsa.GTSA.
Two interchangeable paths:
  * the torch restatement (`forward`, and `realtime_process` on the CPU, with grad enabled, or after use_hip_kernels(False)): plain
    torch ops, differentiable, so train.py can train the model through autograd.  The GRU cell is written out (no nn.GRU forward,
    no MIOpen RNN); the nn.GRU modules only own the parameters;
  * the kernel path (`realtime_process` of a GPU tensor with grad disabled): every segment of a call at once, segment-major as in
    train_net.CRNFunction - the U-Net and the signal chain are train_stages.py's (shared with CRNFunction), the two GRUs
    persistent launches, the beamforming head on csrc/se_gbf.hip.  An unsupported geometry raises ValueError naming the limit; there is no fallback.
  * HIP training (opt-in, use_hip_training(True)): `realtime_process` of a GPU tensor with grad enabled is ONE autograd node,
    GBFFunction - the kernel path's forward keeping its activations, and a backward on the same kernels plus se_gbf_*_bwd.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn
from torch import nn

from . import train_ops as K
from .call_plan import segment_geometry
from .crn import _Deconv, _Norm as _NormParams, _Seq
from .streaming import StreamingMixin
from .train_stages import (_cs, _new, _p, _run, _sig, colsum_tall, decoder_bwd, decoder_fwd, encoder_block_bwd, encoder_block_fwd, gemm_tn,
                           grads_in_parameter_order, gru_layer_bwd, gru_steps, gru_steps_bwd, input_features, istft_into, overlap_add, own_last_slab,
                           start_rows, stft, synthesis_adjoint)

EPS = 1e-8


class _Norm(_NormParams):  # crn.py's GlobalLayerNorm parameter holder, callable: `linear` is an nn.Sequential that runs through its norm
    def forward(self, x):
        return _gln(x, self)


def _gln(x, norm):
    """GlobalLayerNorm(time=False): per-sample statistics over every non-batch dim, denominator sqrt(var + EPS) + EPS."""
    dims = tuple(range(1, x.dim()))
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    return (x - mean) / (torch.sqrt(var + EPS) + EPS) * norm.weight + norm.bias


class _Conv(nn.Module):  # TemporalConv2d, GeneralBeamformer.py:155-205; crn.py's holder has no `padding`, the restatement's time history
    def __init__(self, cin, cout, k, dil, dropout):
        super().__init__()
        self.padding = (k - 1) * dil
        self.conv = nn.Conv2d(cin, cout, (5, k), stride=(2, 1), padding=(2, 0), dilation=(1, dil))
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)
        self.norm = _Norm(cout)


def _gru(x, g, h0):
    """nn.GRU (batch_first) written out: x [N, T, In], h0 [layers, N, H] or None -> (out [N, T, H], hT [layers, N, H])."""
    H = g.hidden_size
    hs = []
    for l in range(g.num_layers):
        gi = x @ getattr(g, f"weight_ih_l{l}").t() + getattr(g, f"bias_ih_l{l}")
        w_hh, b_hh = getattr(g, f"weight_hh_l{l}"), getattr(g, f"bias_hh_l{l}")
        h = h0[l] if h0 is not None else x.new_zeros(x.shape[0], H)
        outs = []
        for t in range(x.shape[1]):
            gh = h @ w_hh.t() + b_hh
            r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
            z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            outs.append(h)
        x = torch.stack(outs, dim=1)
        hs.append(h)
    return x, torch.stack(hs)


class GeneralBeamformer(StreamingMixin, nn.Module):
    def __init__(self, num_channels, num_freqs, hidden, segment_length, num_layers=1, num_inputs=3, kernel_size=3, dropout=0.0,
                 sample_rate=16000, win_length=25, hop_length=10, n_fft=400):
        super().__init__()
        self.segment_length = segment_length
        self.num_freqs = num_freqs
        self.num_time = segment_length // 160 + 1
        self._cfg = dict(num_channels=list(num_channels), hidden=hidden, num_layers=num_layers, num_inputs=num_inputs,
                         kernel_size=kernel_size, sample_rate=sample_rate, win_length=win_length, hop_length=hop_length, n_fft=n_fft)
        # _tstate: dict(buf=[...], hS, hN); _kstate: dict(B, buf=[...], h=[[...], [...]]); taps: xl / phi_s / seq_s / seq_n / w of every
        # forward; max_segments bounds the inference passes only, GBFFunction (training) runs every segment of a call in one pass
        self._init_streaming(num_inputs, sample_rate, win_length, hop_length)
        self._hip_train = False
        L = len(num_channels)
        convs, deconvs = [], []
        for i in range(L):
            cin = (2 * num_inputs - 1) if i == 0 else num_channels[i - 1]
            convs.append(_Conv(cin, num_channels[i], kernel_size, 2 ** i, dropout))
            cout = 4 * num_inputs * 9 if i == 0 else cin
            deconvs.insert(0, _Deconv(num_channels[i], cout, kernel_size, 2 ** (L - i - 1), dropout))
        self.convlist = nn.ModuleList(convs)
        self.deconvlist = nn.ModuleList(deconvs)
        self.ln_S = _Norm(num_freqs * self.num_time)
        self.ln_N = _Norm(num_freqs * self.num_time)
        self.gru_S = _Seq(num_inputs * num_inputs, hidden, num_layers)
        self.gru_N = _Seq(num_inputs * num_inputs, hidden, num_layers)
        self.linear = nn.Sequential(nn.Linear(9, hidden), nn.ReLU(), _Norm(num_freqs), nn.Linear(hidden, 6))

    # ---- reference contract ------------------------------------------------------------------------------------------------
    def compute_loss(self, source, pred_source, length):
        """loss = 0.7 * stoi_loss + 0.3 * (-SI-SNR), NaN -> zeros (GeneralBeamformer.py:500-523); returns (loss, stoi, sisnr)."""
        from .losses import compute_loss
        return compute_loss(source, pred_source, length)

    def forward(self, x):
        """One segment [B, M, F, T, 2] -> [B, F, T, 2] on the torch restatement, carrying the encoder buffers and GRU states."""
        y, self._tstate = self._segment(x, self._tstate)
        return y

    def use_hip_training(self, flag=True):
        """True: realtime_process of a GPU tensor with grad enabled runs forward AND backward on the kernels (GBFFunction), sharing the
        carried state with the inference kernel path.  False (default): grad-enabled calls take the restatement.  Raises ValueError
        at once for a geometry or a dropout setting the training kernels do not cover."""
        if flag:
            err = self.hip_training_error()
            if err:
                raise ValueError(f"GeneralBeamformer HIP training: {err}")
        self._hip_train = bool(flag)
        return self

    def _plan_channels(self, M):
        return [2 * M - 1] + self._cfg["num_channels"]

    def _choose_path(self, mixture):
        grad = torch.is_grad_enabled()
        if self._hip_train and mixture.is_cuda and grad:
            return "train"
        return "kernel" if self._hip and mixture.is_cuda and not grad else "torch"

    def _train_call(self, mixture, plan):
        err = self.hip_training_error()
        if err:
            raise ValueError(f"GeneralBeamformer HIP training: {err}")
        return GBFFunction.apply(self, mixture, plan, *[p for _, p in self.named_parameters()])

    @staticmethod
    def _batch_of(state):
        return state["buf"][0].shape[0]

    # ---- torch restatement ---------------------------------------------------------------------------------------------------
    def _segment(self, x, st):
        B, M, F, T, _ = x.shape
        st = st or dict(buf=None, hS=None, hN=None)
        taps = self.taps
        noisy = x
        re, im = x[..., 0], x[..., 1]
        ang = torch.arctan(im / (re + EPS) + EPS)
        h = torch.cat([torch.sqrt(re ** 2 + im ** 2 + 1e-10), ang[:, :1] - ang[:, 1:]], dim=1)
        residuals, bufs = [h], []
        for i, blk in enumerate(self.convlist):
            P = blk.padding
            buf = st["buf"][i] if st["buf"] is not None else h.new_zeros(B, h.shape[1], h.shape[2], P)
            inp = torch.cat([buf, h], dim=-1)
            bufs.append(inp[..., -P:].detach())
            y = blk.dropout(Fn.conv2d(inp, blk.conv.weight, blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=blk.conv.dilation))
            h = _gln(torch.relu(y), blk.norm)
            residuals.append(h)
        L = len(self.deconvlist)
        for j, blk in enumerate(self.deconvlist):
            y = Fn.conv_transpose2d(h, blk.conv.weight, blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=blk.conv.dilation)
            y = _gln(torch.relu(blk.dropout(y)[..., -T:]), blk.norm)
            if j < L - 1:
                res = residuals[-2 - j]
                if res.shape[2] > y.shape[2]:
                    y = Fn.pad(y, (0, 0, 0, res.shape[2] - y.shape[2]))
                elif res.shape[2] < y.shape[2]:
                    y = y[:, :, :res.shape[2]]
                m = torch.sigmoid(_gln(Fn.conv2d(res, blk.residualmask.weight, blk.residualmask.bias), blk.residualnorm))
                y = m * torch.relu(Fn.conv2d(res, blk.residual.weight, blk.residual.bias)) + (1.0 - m) * y
            h = y
        if taps is not None:
            taps["xl"] = h
        phi = self._head_phi(h, noisy)
        if taps is not None:
            taps["phi_s"] = phi[0]
        yS, hS = self._sequence(self.gru_S, phi[0].reshape(B * F, T, 9), st["hS"])
        yN, hN = self._sequence(self.gru_N, phi[1].reshape(B * F, T, 9), st["hN"])
        if taps is not None:
            taps["seq_s"], taps["seq_n"] = yS.transpose(1, 2), yN.transpose(1, 2)   # the reference layout [B*F, 9, T]
        w = self.linear((yS * yN).reshape(B, F, T, 9)).reshape(B, F, T, M, 2)  # .conj() of a real tensor: a no-op
        if taps is not None:
            taps["w"] = w
        Y = self._beamform(w, noisy)
        return Y, dict(buf=bufs, hS=hS.detach(), hN=hN.detach())

    def _head_phi(self, xl, noisy):
        """xl [B, 4M*9, F, T] -> (Phi_S, Phi_N) after ln_S / ln_N, [B, F*T, M, M] (GeneralBeamformer.py:336-357)."""
        B, M, F, T, _ = noisy.shape
        f5 = xl.reshape(B, 2, 2, M, 9, F * T)
        u = Fn.unfold(noisy.reshape(B, M, F, T * 2), (3, 3), padding=1).reshape(B, M, 9, F * T, 2)
        ur, ui = u[..., 0], u[..., 1]
        out = []
        for q, ln in ((0, self.ln_S), (1, self.ln_N)):
            fr, fi = f5[:, q, 0], f5[:, q, 1]
            sr = (fr * ur - fi * ui).sum(dim=2).transpose(1, 2)   # [B, F*T, M]
            si = (fr * ui + fi * ur).sum(dim=2).transpose(1, 2)
            phi = sr[..., :, None] * sr[..., None, :] + si[..., :, None] * si[..., None, :]
            out.append(_gln(phi, ln))
        return out

    @staticmethod
    def _beamform(w, noisy):
        n = noisy.permute(0, 2, 3, 1, 4)  # [B, F, T, M, 2]
        real = w[..., 0] * n[..., 0] - w[..., 1] * n[..., 1]
        img = w[..., 0] * n[..., 1] + w[..., 1] * n[..., 0]
        return torch.stack([real, img], dim=-1).sum(dim=-2)

    @staticmethod
    def _sequence(sm, x, h0):
        """SequenceModel.forward on [B*F, T, 9] rows: GRU, fc, ReLU, gLN over T x 9 -> ([B*F, T, 9], hT)."""
        o, hT = _gru(x, sm.sequence_model, h0)
        o = torch.relu(sm.fc_output_layer(o))
        return _gln(o.unsqueeze(1), sm.norm).squeeze(1), hT

    def _torch_windows(self, X, st):
        outs = []
        for n in range(X.shape[2]):
            y, st = self._segment(X[:, :, n], st)
            outs.append(y)
        return torch.stack(outs, dim=1), st

    def _state_row(self, st, b, B):
        F = self.num_freqs   # hS / hN: [layers, B * F, H]
        return dict(buf=[t[b:b + 1] for t in st["buf"]], hS=st["hS"][:, b * F:(b + 1) * F], hN=st["hN"][:, b * F:(b + 1) * F])

    def _state_merge(self, rows):
        return dict(buf=[torch.cat([r["buf"][i] for r in rows]) for i in range(len(self.convlist))],
                    hS=torch.cat([r["hS"] for r in rows], dim=1), hN=torch.cat([r["hN"] for r in rows], dim=1))

    # ---- kernel path ---------------------------------------------------------------------------------------------------------
    def kernel_geometry_error(self):
        """None when the kernel path supports this geometry, else the limit that fails (realtime_process raises it as ValueError)."""
        c = self._cfg
        M, k, H, ch = c["num_inputs"], c["kernel_size"], c["hidden"], [2 * c["num_inputs"] - 1] + c["num_channels"]
        Lv = len(c["num_channels"])
        geo = segment_geometry(0, False, self.segment_length, self._hop, c["n_fft"], ch)
        T, F0, Fq = geo["T"], geo["F0"], geo["Fq"]
        if M != 3:
            return f"num_inputs = {M}: the beamforming head's linear layers are 9 -> hidden -> 6, so 3 microphones only"
        if k != 3:
            return f"kernel_size = {k}: the convolution kernels are 5 x 3"
        if F0 != self.num_freqs or T != self.num_time:
            return f"STFT gives {F0} x {T} bins, the model is built for {self.num_freqs} x {self.num_time} (ln_S / ln_N weights)"
        if T > 64:
            return f"{T} frames per segment: the sequence head takes at most 64"
        for what, co in [(f"convlist.{i}", ch[i + 1]) for i in range(Lv)] + [(f"deconvlist.{Lv - 1}", 4 * M * 9)]:
            if (co + 31) // 32 * 32 not in (32, 64, 128):
                return f"{what}: {co} output channels do not pad to 32, 64 or 128 (the conv kernels' GEMM rows)"
        if not K._lib().se_train_gru_pseq_supported(1, H):
            return f"hidden = {H}: no persistent GRU kernel (se_train_gru_pseq_supported)"
        if (k - 1) * 2 ** (Lv - 1) >= T:
            return f"encoder history (k - 1) * 2^(L - 1) = {(k - 1) * 2 ** (Lv - 1)} frames is not shorter than the {T}-frame segment"
        for j in range(Lv - 1):
            kk = Lv - 1 - j
            if Fq[kk] < 2 * Fq[kk + 1] - 1:
                return f"deconvlist.{j}: {2 * Fq[kk + 1] - 1} frequencies do not fit the {Fq[kk]}-bin skip tensor"
        if 2 * Fq[1] - 1 != self.num_freqs:
            return f"last decoder block gives {2 * Fq[1] - 1} frequencies, num_freqs = {self.num_freqs}"
        return None

    def _padded_w_ih(self, g):
        """W_ih_l0 [3H][9] zero-padded to [3H][16] (the GEMM's K % 8), once per parameter version."""
        w = g.weight_ih_l0
        return self._cached(("w_ih", id(g)), [w], lambda: Fn.pad(w.float(), (0, 16 - w.shape[1])))

    def hip_training_error(self):
        """None when GBFFunction can train this model as it stands, else the limit that fails (geometry, or active dropout)."""
        err = self.kernel_geometry_error()
        if err:
            return err
        if self.training and any(b.dropout.p > 0 for b in list(self.convlist) + list(self.deconvlist)):
            return "dropout is active in training mode: the training kernels have no dropout (use the restatement, or dropout = 0)"
        return None

    def _kernel_setup(self, mixture, plan):
        """The sizes of one realtime_process call on the kernels (the plan's geometry and the model's own) and the state it starts from:
        zeros, or the carried one - row b of it where flags[b], zeros elsewhere, for a batch of chunk chains."""
        dev = mixture.device
        B, M, L = mixture.shape
        c = self._cfg
        H, NL = c["hidden"], c["num_layers"]
        T, F0, ch, Fq, Lv = plan.T, plan.F0, plan.ch, plan.Fq, len(self.convlist)
        g = dict(plan.geo, plan=plan, L=L, B=B, M=M, n_fft=c["n_fft"], H=H, NL=NL, Lv=Lv, BF=B * F0,
                 sig=_sig(dev, c["n_fft"], self._win, self._hop, self.segment_length))
        state = self._kstate if plan.any_flag else None   # realtime_process has refused a state of another batch size
        if state is not None:
            state = dict(B=B, buf=[start_rows(plan, t) for t in state["buf"]], h=[[start_rows(plan, t) for t in hq] for hq in state["h"]])
        else:
            state = dict(B=B, buf=[torch.zeros(B, ch[i], T, Fq[i], device=dev) for i in range(Lv)],
                         h=[[torch.zeros(B * F0, H, device=dev) for _ in range(NL)] for _ in range(2)])
        return g, state

    def _kernel_pass(self, mixture, g, state, n0, Nc, yseg, tmo, sv=None):
        """Segments [n0, n0 + Nc) of the call: STFT, U-Net, head, GRUs, iSTFT into yseg; advances `state`.  sv (a dict): also keep
        what GBFFunction.backward needs (GRU gates, layer outputs, the U-Net activations and gLN / skip statistics)."""
        lib = K._lib()
        dev = mixture.device
        st = K._st
        B, M, L, T, F0, H, NL, Lv, ch, Fq, BF, P = (g[k] for k in ("B", "M", "L", "T", "F0", "H", "NL", "Lv", "ch", "Fq", "BF", "P"))
        S = Nc * B
        keep = sv is not None
        plan = g["plan"]
        # chunk chains: utterance b has live[b] of this pass's Nc segments; its GRU streams run live[b] * T steps
        steps, live = gru_steps(plan, dev, T, F0, n0, Nc)
        spec = stft(plan, g["sig"], mixture, M, n0, Nc)
        # encoder: xin[i] = [Nc + 1][B][C][T][F], slab 0 = the carried input of block i (its time history)
        xin = []
        for i in range(Lv):
            t_ = _new(Nc + 1, B, ch[i], T, Fq[i], dev=dev)
            t_[0].copy_(state["buf"][i])
            xin.append(t_)
        input_features(spec, xin[0], S, B, M, ch[0], T, F0)
        ys, stats_e = [], []
        for i, blk in enumerate(self.convlist):
            Co, Fo = ch[i + 1], Fq[i + 1]
            if i == Lv - 1:
                xin.append(_new(S, Co, T, Fo, dev=dev))   # the decoder's input: no history slab
            y_st = encoder_block_fwd(blk, xin[i], _p(xin[i + 1], B * Co * T * Fo if i < Lv - 1 else 0), _cs(Co, T, Fo), S, B, ch[i], Co, T, Fq[i], Fo, 2 ** i)
            if keep:
                ys.append(y_st[0])
                stats_e.append(y_st[1])
        del y_st
        xl, dec = decoder_fwd(self.deconvlist, xin, ch, Fq, S, B, T, 1, 0, keep=keep, stacked=False)
        # head: PSD + ln -> GRU rows [B*F][Nc*T][16] (stream-major), two GRU models, sequence head, beamformer
        R, TT = BF * Nc * T, Nc * T
        rows = [_new(R, 16, dev=dev), _new(R, 16, dev=dev)]
        _run("k_gbf_psd", 0.0, lib.se_gbf_psd_fwd, _p(xl), _p(spec), _p(self.ln_S.weight), _p(self.ln_S.bias), _p(self.ln_N.weight),
             _p(self.ln_N.bias), _p(rows[0]), _p(rows[1]), S, B, M, T, F0, st())
        models = (self.gru_S, self.gru_N)
        last, outs, gates, h0s = [], [[], []], [[], []], [[], []]
        for q, m in enumerate(models):
            gm = m.sequence_model
            x_l = rows[q]
            for l in range(NL):
                gi = K._gemm(x_l, self._padded_w_ih(gm) if l == 0 else getattr(gm, f"weight_ih_l{l}"), getattr(gm, f"bias_ih_l{l}"))
                out = _new(R, H, dev=dev)
                gt = _new(R, 4 * H, dev=dev) if keep else None
                hT = _new(BF, H, dev=dev)
                sc = K._gru_seq_fwd(gi, state["h"][q][l], getattr(gm, f"weight_hh_l{l}"), getattr(gm, f"bias_hh_l{l}"), out, gt, hT, BF, TT, H, TT, 0, TT,
                                    tag=("gbf", q, l), steps=steps)
                tmo.append(sc[:2].view(torch.int32)[1:2].clone())   # this launch's timeout word, before the next launch's memset
                del gi
                if keep:
                    outs[q].append(out)
                    gates[q].append(gt)
                    h0s[q].append(state["h"][q][l])
                state["h"][q][l] = hT
                x_l = out
            last.append(x_l)
        if not keep:
            del rows
        phi = _new(S, F0, T, 9, dev=dev)
        sS, sN = self.gru_S, self.gru_N
        _run("k_gbf_seq", 0.0, lib.se_gbf_seq_fwd, _p(last[0]), _p(last[1]), _p(sS.fc_output_layer.weight), _p(sS.fc_output_layer.bias),
             _p(sS.norm.weight), _p(sS.norm.bias), _p(sN.fc_output_layer.weight), _p(sN.fc_output_layer.bias), _p(sN.norm.weight),
             _p(sN.norm.bias), _p(phi), None, None, S, B, F0, T, H, st())
        del last
        Y = _new(S, T, F0, 2, dev=dev)
        lin = self.linear
        _run("k_gbf_bf", 0.0, lib.se_gbf_bf_fwd, _p(phi), _p(spec), _p(lin[0].weight), _p(lin[0].bias), _p(lin[2].weight), _p(lin[2].bias),
             _p(lin[3].weight), _p(lin[3].bias), _p(Y), None, S, M, T, F0, H, st())
        istft_into(plan, g["sig"], Y, yseg, n0, Nc)   # every stream in every pass: one launch
        # every utterance's own last live segment of the pass; slab 0 (its previous rows) where it has none
        state["buf"] = [own_last_slab(plan, xin[i], live, copy=True) for i in range(Lv)]
        if keep:
            sv.update(spec=spec, xin=xin, ys=ys, stats_e=stats_e, dec=dec, xl=xl, rows=rows, outs=outs, gates=gates, h0s=h0s, phi=phi)

    def _check_timeouts(self, tmo, g):
        if tmo and int(torch.cat(tmo).abs().sum()) != 0:
            self._kstate = None
            raise RuntimeError(f"persistent GRU kernel timed out waiting for its peer workgroups ({g['BF']} streams, hidden {g['H']}): "
                               "output invalid")

    def _kernel_run(self, mixture, plan, sv=None):
        """Passes of max_segments segments; sv given (GBFFunction): ONE pass that keeps its activations.  -> (pred, geometry, time-outs)"""
        g, state = self._kernel_setup(mixture, plan)
        N, B = g["N"], g["B"]
        yseg = _new(N, B, g["Ks"], dev=mixture.device)
        tmo = []
        step = N if sv is not None else max(1, int(self.max_segments))
        for n0 in range(0, N, step):
            self._kernel_pass(mixture, g, state, n0, min(step, N - n0), yseg, tmo, sv)
        pred = overlap_add(plan, g["sig"], yseg)
        self._kstate = state
        return pred, g, tmo

    @torch.no_grad()
    def _kernel_process(self, mixture, plan):
        if self.training and any(b.dropout.p > 0 for b in list(self.convlist) + list(self.deconvlist)):
            raise ValueError("GeneralBeamformer kernel path: inference only (dropout is active in training mode; use the restatement)")
        pred, g, tmo = self._kernel_run(mixture, plan)
        self._check_timeouts(tmo, g)
        return pred


class GBFFunction(torch.autograd.Function):
    """pred = GeneralBeamformer.realtime_process(mixture, flag) on the kernels, forward AND backward, as one autograd node
    (reference training step train.py:195-204).  forward(ctx, model, mixture, plan, *params), params in named_parameters() order;
    plan: the call's CallPlan (realtime_process builds it).

    Forward: the inference kernel path over all N segments of the call in one pass, keeping the GRU gates, layer outputs and U-Net
    activations.  Backward: OLA / iSTFT adjoint, se_gbf_bf_bwd, se_gbf_seq_bwd, the GRU layers (train_stages.gru_layer_bwd),
    se_gbf_psd_bwd, then train_stages.decoder_bwd and encoder_block_bwd, the passes CRNFunction runs.  The reference detaches h at every segment seam
    (GeneralBeamformer.py:143), so each GRU layer's BPTT is ONE persistent launch over B*F*N independent streams of T steps.  No
    float atomics: the gradients are bit-reproducible."""

    @staticmethod
    def forward(ctx, model, mixture, plan, *params):
        K._need_gpu(mixture, model.ln_S.weight)
        sv = {}
        pred, g, tmo = model._kernel_run(mixture.detach().contiguous().float(), plan, sv)
        g["S"] = g["N"] * g["B"]
        ctx.model, ctx.dims, ctx.sv, ctx.tmo = model, g, sv, tmo
        return pred

    @staticmethod
    def backward(ctx, dpred):
        lib = K._lib()
        model, q, sv, tmo = ctx.model, ctx.dims, ctx.sv, list(ctx.tmo)
        B, M, N, S, T, F0, Ks, H, NL, Lv, BF = (q[k] for k in ("B", "M", "N", "S", "T", "F0", "Ks", "H", "NL", "Lv", "BF"))
        ch, Fq, sig = q["ch"], q["Fq"], q["sig"]
        dev = dpred.device
        st = K._st
        dpred = dpred.contiguous().float()
        grads = {}
        zero_bias = torch.zeros(256, device=dev)

        dY = synthesis_adjoint(q["plan"], sig, dpred)
        steps = gru_steps_bwd(q["plan"], dev, T, F0)   # chunk chains: a sequence of the GRU sweep is one (stream, segment) pair
        # beamformer + linear head
        FT = F0 * T
        R1 = S * FT
        lin = model.linear
        dphi = _new(S, F0, T, 9, dev=dev)
        dpre, act, dw = _new(R1, H, dev=dev), _new(R1, H, dev=dev), _new(R1, 8, dev=dev)
        pg, pb = _new(S * T, F0, dev=dev), _new(S * T, F0, dev=dev)
        _run("k_gbf_bf_bwd", 0.0, lib.se_gbf_bf_bwd, _p(dY), _p(sv["phi"]), _p(sv["spec"]), _p(lin[0].weight), _p(lin[0].bias), _p(lin[2].weight),
             _p(lin[2].bias), _p(lin[3].weight), _p(dphi), _p(dpre), _p(act), _p(dw), _p(pg), _p(pb), S, M, T, F0, H, q["n_fft"], st())
        grads["linear.0.weight"] = gemm_tn(dpre, sv["phi"].view(R1, 9))
        grads["linear.0.bias"] = colsum_tall(dpre)
        grads["linear.3.weight"] = gemm_tn(dw, act)[:6]
        grads["linear.3.bias"] = colsum_tall(dw)[:6]
        grads["linear.2.weight"], grads["linear.2.bias"] = colsum_tall(pg), colsum_tall(pb)
        del dY, dpre, act, dw, pg, pb
        # sequence heads: fc + ReLU + gLN of both models, and their product
        R = BF * N * T
        outs, gates, h0s, rows = sv["outs"], sv["gates"], sv["h0s"], sv["rows"]
        models = (("gru_S", model.gru_S), ("gru_N", model.gru_N))
        dh = [_new(R, H, dev=dev), _new(R, H, dev=dev)]
        dv = [_new(R, 16, dev=dev), _new(R, 16, dev=dev)]
        part = _new(S * F0, 54, dev=dev)
        sS, sN = model.gru_S, model.gru_N
        _run("k_gbf_seq_bwd", 0.0, lib.se_gbf_seq_bwd, _p(dphi), _p(outs[0][NL - 1]), _p(outs[1][NL - 1]), _p(sS.fc_output_layer.weight),
             _p(sS.fc_output_layer.bias), _p(sS.norm.weight), _p(sS.norm.bias), _p(sN.fc_output_layer.weight), _p(sN.fc_output_layer.bias),
             _p(sN.norm.weight), _p(sN.norm.bias), _p(dh[0]), _p(dh[1]), _p(dv[0]), _p(dv[1]), _p(part), S, B, F0, T, H, st())
        del dphi
        ps = colsum_tall(part)
        for qi, (name, sm) in enumerate(models):
            o = qi * 27
            grads[name + ".norm.weight"], grads[name + ".norm.bias"] = ps[o:o + 9], ps[o + 9:o + 18]
            grads[name + ".fc_output_layer.bias"] = ps[o + 18:o + 27]
            grads[name + ".fc_output_layer.weight"] = gemm_tn(dv[qi], outs[qi][NL - 1])[:9]
        del dv
        # the GRU layers in reverse: the state is detached at every seam, so B*F*N independent streams of T steps per launch
        drows = []
        for qi, (name, sm) in enumerate(models):
            gm = sm.sequence_model
            dlayer = dh[qi]
            for l in range(NL - 1, -1, -1):
                w_ih = model._padded_w_ih(gm) if l == 0 else getattr(gm, f"weight_ih_l{l}")
                x_l = rows[qi] if l == 0 else outs[qi][l - 1]
                dlayer = gru_layer_bwd(dlayer, outs[qi][l], gates[qi][l], h0s[qi][l], x_l, w_ih, getattr(gm, f"weight_hh_l{l}"),
                                       f"{name}.sequence_model.", l, grads, BF, N, T, H, N * T, 0, N * T, tag=("gbf_bwd", qi, l), tmo=tmo, steps=steps)
                if l == 0:   # [3H][16] against the padded rows: the parameter is [3H][9]; dlayer [R][16] = the gradient of the GRU input rows
                    grads[f"{name}.sequence_model.weight_ih_l0"] = grads[f"{name}.sequence_model.weight_ih_l0"][:, :9].contiguous()
            drows.append(dlayer)
        del dh
        # PSD + ln_S / ln_N
        dxl = torch.empty_like(sv["xl"])
        part = _new(S, 4 * FT, dev=dev)
        _run("k_gbf_psd_bwd", 0.0, lib.se_gbf_psd_bwd, _p(sv["xl"]), _p(sv["spec"]), _p(model.ln_S.weight), _p(model.ln_S.bias),
             _p(model.ln_N.weight), _p(model.ln_N.bias), _p(drows[0]), _p(drows[1]), _p(dxl), _p(part), S, B, M, T, F0, st())
        del drows
        pp = colsum_tall(part)
        grads["ln_S.weight"], grads["ln_S.bias"] = pp[:FT], pp[FT:2 * FT]
        grads["ln_N.weight"], grads["ln_N.bias"] = pp[2 * FT:3 * FT], pp[3 * FT:]
        dout, dres = decoder_bwd(model.deconvlist, sv["dec"], sv["xin"], dxl, grads, zero_bias, S, B, T, 1, 0, stacked=False)
        del dxl
        # encoder, last block first
        dy_ptr, ds = _p(dout), _cs(ch[Lv], T, Fq[Lv])
        for i in range(Lv - 1, -1, -1):
            dout = encoder_block_bwd(model.convlist[i], f"convlist.{i}.", grads, dy_ptr, ds, sv["ys"][i], sv["stats_e"][i], sv["xin"][i], dres.get(i),
                                     zero_bias, S, B, ch[i], ch[i + 1], T, Fq[i], Fq[i + 1], 2 ** i, need_dx=i > 0)  # the features carry no gradient
            if i:
                dy_ptr, ds = _p(dout), _cs(ch[i], T, Fq[i])
        ctx.sv = ctx.tmo = None
        model._check_timeouts(tmo, q)
        return (None, None, None, *grads_in_parameter_order(model, grads))
