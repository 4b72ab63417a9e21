"""Trainable FullSubNet: the reference trainer's loop (train_fullsubnet.py:137-145) on the drop-in model.

    pred_source, pred_crm, sf, xf = model.realtime_process(mixture, source, data['flag'], train=False)
    loss, logmse, sisnr = model.compute_loss(source[:, 0], pred_source, xf, sf, pred_crm, length)
    scaler.scale(loss / gradient_accumulation).backward()

`TrainableFullSubNet` has the constructor, state_dict and compute_loss of `fullsubnet.FullSubNet`, and two interchangeable
differentiable forwards of `realtime_process(train=False)` (fullsubnet.py:903-961, one forward per 3200-sample window,
fullsubnet.py:769-824):
  * `use_hip_kernels(True)`: ONE autograd node (`FSNFunction`): STFT, both LSTMs, the mask, iSTFT and overlap-add forward and
    backward on the hand-written kernels (fsn_train_fwd / fsn_train_bwd + se_sig_* / se_train_*; no float atomics);
  * default: a torch-autograd restatement with the LSTM cell written out (matmul + sigmoid / tanh per step, no nn.LSTM and so no
    MIOpen RNN), CPU-runnable and dtype-generic - the checker, pinned to the reference by tests/golden/fsn_grad_golden.npz.
What the reference detaches, both paths detach: the LSTM states after every window (fullsubnet.py:819-820: the BPTT stops at each
window seam) and both CumLayerNorm running means (fullsubnet.py:200: the norm's gradient is 1 / (mean + EPS) of the window).
Under torch.no_grad() on the GPU, realtime_process takes FullSubNet's inference engine.  train=True keeps FullSubNet's forward-only
single pass.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import train_ops as K
from .fullsubnet import FullSubNet
from .train_stages import _as_flag, _sig, segment_geometry, stft, synthesis, synthesis_adjoint
from .training import _TrainableMixin

EPS = 1e-8  # fullsubnet.py:12


class FSNFunction(torch.autograd.Function):
    """pred = realtime_process(mixture, flag, train=False)[0] on the kernels.  forward(ctx, model, mixture, flag, *params) with params
    in state_dict order (what fsn_train_bwd writes)."""

    @staticmethod
    def forward(ctx, model, mixture, flag, *params):
        K._need_gpu(mixture, params[0])
        eng = model._engine_for(mixture)  # (re)loads the weights when an optimizer step changed them
        g = model._geometry(mixture)
        B, M, L, N, T, F = g["B"], g["M"], g["L"], g["N"], g["T"], g["F"]
        dev = mixture.device
        mixture = mixture.contiguous().float()
        S = N * B
        spec = stft(g["sig"], mixture, B, M, L, g["off0"], g["P"], N, T, F)
        ws = torch.empty(eng.train_ws_bytes(B, N), dtype=torch.uint8, device=dev)
        crm = eng.train_fwd(spec, B, N, flag, ws)                                # [N, B, 2, F, T]
        xm = crm.permute(0, 1, 2, 4, 3).reshape(S, 2, T, F).contiguous()
        Y = torch.empty(S, T, F, 2, device=dev)
        K._chk(K._lib().se_train_mask_fwd(xm.data_ptr(), spec.data_ptr(), Y.data_ptr(), S, M, T, F, K._st()))
        pred = synthesis(g["sig"], Y, B, g["Ks"], L, g["skip"])
        model._hip_aux = (crm, spec)
        ctx.eng, ctx.ws, ctx.spec, ctx.xm, ctx.g = eng, ws, spec, xm, g
        ctx.shapes = [p.shape for p in params]
        return pred

    @staticmethod
    def backward(ctx, dpred):
        g = ctx.g
        B, M, L, N, T, F = g["B"], g["M"], g["L"], g["N"], g["T"], g["F"]
        S, dev = N * B, dpred.device
        dY = synthesis_adjoint(g["sig"], dpred.contiguous().float(), B, N, L, g["skip"], g["Ks"], T, F)
        dx = torch.empty(S, 2, T, F, device=dev)
        K._chk(K._lib().se_train_mask_bwd(dY.data_ptr(), ctx.xm.data_ptr(), ctx.spec.data_ptr(), dx.data_ptr(), S, M, T, F, g["n_fft"], K._st()))
        dcrm = dx.view(N, B, 2, T, F).permute(0, 1, 2, 4, 3).contiguous()
        grads = [torch.empty(s, device=dev) for s in ctx.shapes]
        ctx.eng.train_bwd(dcrm, B, N, ctx.ws, grads)
        ctx.ws = ctx.spec = ctx.xm = None
        return (None, None, None, *grads)


class TrainableFullSubNet(FullSubNet):
    """fullsubnet.FullSubNet with a differentiable realtime_process(train=False); same constructor, state_dict and compute_loss."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        a_ = self._args
        self._win = int(round(a_["sample_rate"] / 1000.0 * a_["win_length"]))
        self._hop = int(round(a_["sample_rate"] / 1000.0 * a_["hop_length"]))
        self._nfft = a_["n_fft"]
        self._hip = False
        self._tstate = None   # the restatement's carried state (LSTM states, running means, step counters)
        self._hip_aux = None

    def use_hip_kernels(self, flag=True):
        """True: FSNFunction (the kernels, forward and backward); False (default): the torch restatement (the checker).  The two
        paths carry their state separately: start with flag=False after switching."""
        self._hip = bool(flag)
        self._tstate = None
        return self

    def _geometry(self, mixture, flag=None):
        B, M, L = mixture.shape
        n_fft, Ks = self._args["n_fft"], self.segment_length
        g = segment_geometry(L, self._cur_flag if flag is None else flag, Ks, self._hop, n_fft)
        g.update(B=B, M=M, n_fft=n_fft, F=self.num_freqs, sig=_sig(mixture.device, n_fft, self._win, self._hop, Ks))
        return g

    def realtime_process(self, mixture, source=None, flag=False, train=False):
        if train:
            return super().realtime_process(mixture, source, flag, True)
        flag = _as_flag(flag)
        if not torch.is_grad_enabled() and mixture.is_cuda:
            return super().realtime_process(mixture, source, flag, False)
        self._cur_flag = flag
        if self._hip:
            pred, crm, x = self._hip_forward(mixture, flag)
            s = None if source is None else self._mic0_spec(source, flag)
        else:
            pred, crm, x, s = self._torch_forward(mixture, source, flag)
        if source is None:
            return pred
        return pred, crm.detach(), s.detach(), x.detach()

    # ---- kernels ----
    def _hip_forward(self, mixture, flag):
        params = list(self.parameters())
        pred = FSNFunction.apply(self, mixture, flag, *params)
        crm, spec = self._hip_aux
        self._hip_aux = None
        g = self._geometry(mixture, flag)
        N, B, M, T, F = g["N"], g["B"], g["M"], g["T"], g["F"]
        x0 = spec.view(N, B, M, T, F, 2)[:, :, 0].permute(0, 1, 4, 3, 2).contiguous()  # [N, B, 2, F, T]
        return pred, crm, x0

    def _mic0_spec(self, source, flag):
        src = source[:, :1].contiguous().float()
        g = self._geometry(src, flag)
        sspec = stft(g["sig"], src, g["B"], 1, g["L"], g["off0"], g["P"], g["N"], g["T"], g["F"])   # [N, B, T, F, 2]
        return sspec.permute(0, 1, 4, 3, 2).contiguous()

    # ---- torch restatement (the checker) ----
    _segment = _TrainableMixin._segment
    _stft = _TrainableMixin._stft
    _istft = _TrainableMixin._istft

    @staticmethod
    def _lstm(x, layers, state):
        """x [R, T, In]; layers = [(W_ih, W_hh, b_ih, b_hh)]; state = [(h, c)] per layer or None -> out [R, T, H], detached new state."""
        new = []
        for l, (wih, whh, bih, bhh) in enumerate(layers):
            H = whh.shape[1]
            if state is None:
                h = x.new_zeros(x.shape[0], H)
                c = x.new_zeros(x.shape[0], H)
            else:
                h, c = state[l]
            xw = torch.matmul(x, wih.t()) + (bih + bhh)
            outs = []
            for t in range(x.shape[1]):
                gt = xw[:, t] + torch.matmul(h, whh.t())
                i, f, g, o = gt.chunk(4, dim=1)
                i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                c = f * c + i * g
                h = o * torch.tanh(c)
                outs.append(h)
            x = torch.stack(outs, dim=1)
            new.append((h.detach(), c.detach()))
        return x, new

    @staticmethod
    def _cumnorm(x, st, key):
        """CumLayerNorm (fullsubnet.py:184-201): x / (running mean + EPS), the running mean detached."""
        mean = x.detach().mean(dim=(1, 2, 3), keepdim=True)
        rm, step = st.get(key), st.get(key + "_step", 0)
        rm = mean if rm is None else (step / (step + 1)) * rm + (1.0 - step / (step + 1)) * mean
        st[key], st[key + "_step"] = rm, min(step + 1, 80)
        return x / (rm + EPS)

    def _layers(self, seq):
        m = seq.sequence_model
        return [(getattr(m, f"weight_ih_l{l}"), getattr(m, f"weight_hh_l{l}"), getattr(m, f"bias_ih_l{l}"), getattr(m, f"bias_hh_l{l}"))
                for l in range(m.num_layers)]

    def _torch_window(self, X, st):
        """FullSubNet.forward (fullsubnet.py:769-824) of one window: X [B, M, F, T] complex -> crm [B, 2, F, T]."""
        B, M, F, T = X.shape
        nb = self._args["sb_neighbors"]
        noisy = torch.sqrt(X.real ** 2 + X.imag ** 2 + EPS)
        noisy = self._cumnorm(noisy, st, "mean_fb")
        fb_in = noisy.reshape(B, M * F, T).transpose(1, 2)
        fb_h, st["fh"] = self._lstm(fb_in, self._layers(self.fb_model), st.get("fh"))
        fb_out = torch.relu(Fn.linear(fb_h, self.fb_model.fc_output_layer.weight, self.fb_model.fc_output_layer.bias))  # [B, T, F]
        idx = torch.arange(F, device=X.device)[:, None] + torch.arange(-nb, nb + 1, device=X.device)[None, :]
        idx = idx.abs()
        idx = torch.where(idx >= F, 2 * (F - 1) - idx, idx)  # reflect pad (fullsubnet.py:322)
        unf = noisy[:, 0][:, idx, :]                             # [B, F, 2nb+1, T]
        sb_in = torch.cat([unf, fb_out.transpose(1, 2).unsqueeze(2)], dim=2)
        sb_in = self._cumnorm(sb_in, st, "mean_sb")
        x = sb_in.reshape(B * F, sb_in.shape[2], T).transpose(1, 2)
        sb_h, st["sh"] = self._lstm(x, self._layers(self.sb_model), st.get("sh"))
        m = Fn.linear(sb_h, self.sb_model.fc_output_layer.weight, self.sb_model.fc_output_layer.bias)  # [B*F, T, 2]
        return m.reshape(B, F, T, 2).permute(0, 3, 1, 2)

    def _torch_forward(self, mixture, source, flag):
        K_ = self.segment_length
        P = K_ // 2
        M = mixture.shape[1]
        if not flag:
            mixture = Fn.pad(mixture, (P, 0))
            self._tstate = {}
        elif self._tstate is None:
            raise RuntimeError("flag=True continues a previous chunk of this path: start with flag=False")
        seg, gap = self._segment(mixture)   # [B, M, N, K]
        X = self._stft(seg)                 # [B, M, N, F, T]
        st = self._tstate
        crms = [self._torch_window(X[:, :, n], st) for n in range(X.shape[2])]
        crm = torch.stack(crms, dim=0)      # [N, B, 2, F, T]
        m = 9.9 * (crm >= 9.9) - 9.9 * (crm <= -9.9) + crm * (crm.abs() < 9.9)  # decompress_cIRM, utility.py:439-442
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        X0 = X[:, 0].transpose(0, 1)        # [N, B, F, T]
        re, im = X0.real, X0.imag
        Y = torch.complex(m[:, :, 0] * re - m[:, :, 1] * im, m[:, :, 1] * re + m[:, :, 0] * im)
        y = self._istft(Y).transpose(0, 1)  # [B, N, K]
        B = y.shape[0]
        s1 = y[:, 0::2].reshape(B, -1)[:, P:]
        s2 = y[:, 1::2].reshape(B, -1)[:, :-P]
        out = (s1 + s2) / 2
        if gap > 0:
            out = out[:, :-gap]
        pred = out if flag else out[:, P:]
        x0 = torch.stack([re, im], dim=2)
        s0 = None
        if source is not None:
            src = source if flag else Fn.pad(source, (P, 0))
            S0 = self._stft(self._segment(src[:, :1])[0])[:, 0].transpose(0, 1)
            s0 = torch.stack([S0.real, S0.imag], dim=2)
        return pred, crm, x0, s0
