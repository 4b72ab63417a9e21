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

Batched chunk chains (datagen.ChunkChainBatch): `flag` with one value per utterance and / or `lengths` make the batch B independent
chains, the contract of fsn_realtime_process_chains and of CRN chain training: utterance b is mixture[b, :, :lengths[b]] (zero beyond,
whatever the padding holds), starts from zero state, reset norms and the K/2 lead where flag[b] is False, continues row b of the
carried state where it is True; pred[b, lengths[b]:] = 0; crm / x / s cover all N = max N_b windows, crm with exact zeros in the
windows past an utterance's own last one; afterwards every utterance holds the state it alone would carry.  Both forwards honour it
(fsn_train_*_chains on the kernels: a fresh batch is sorted by window count and its workspace packed).  A batch whose
flags are all alike and whose lengths are all Lmax takes the scalar path, as a bool flag does.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import train_ops as K
from .fullsubnet import FullSubNet
from .train_stages import (_as_flag, _as_flags, _as_lengths, _rows, _sig, ragged_geometry, segment_geometry, stft, stft_rows, synthesis,
                           synthesis_adjoint, synthesis_adjoint_rows, synthesis_rows)
from .training import _TrainableMixin

EPS = 1e-8  # fullsubnet.py:12


def _x0(spec, N, B, M, T, F):
    """mic 0 of spec [N][B*M][T][F][2] in the reference's layout [N, B, 2, F, T]"""
    return spec.view(N, B, M, T, F, 2)[:, :, 0].permute(0, 1, 4, 3, 2).contiguous()


class FSNFunction(torch.autograd.Function):
    """pred = realtime_process(mixture, flag, train=False)[0] on the kernels.  forward(ctx, model, mixture, flag, *params) with params
    in state_dict order (what fsn_train_bwd writes).  flag: a bool, or (flags, lengths) - B bools and B ints, host values - of a batch
    of chunk chains (fsn_train_*_chains)."""

    @staticmethod
    def forward(ctx, model, mixture, flag, *params):
        K._need_gpu(mixture, params[0])
        eng = model._engine_for(mixture)  # (re)loads the weights when an optimizer step changed them
        mixture = mixture.contiguous().float()
        B, M, L = mixture.shape
        if not isinstance(flag, tuple) and flag and eng._order is not None and len(eng._order) == B:
            flag = ((True,) * B, (L,) * B)  # the carried batch was permuted by a chains call: keep the caller's row b on its utterance
        ctx.shapes = [p.shape for p in params]
        if isinstance(flag, tuple):
            return FSNFunction._forward_chains(ctx, model, eng, mixture, list(flag[0]), list(flag[1]))
        g = model._geometry(mixture, flag)
        N, T, F = g["N"], g["T"], g["F"]
        dev = mixture.device
        S = N * B
        spec = stft(g["sig"], mixture, B, M, L, g["off0"], g["P"], N, T, F)
        ws = torch.empty(eng.train_ws_bytes(B, N), dtype=torch.uint8, device=dev)
        crm = eng.train_fwd(spec, B, N, flag, ws)                                # [N, B, 2, F, T]
        xm = crm.permute(0, 1, 2, 4, 3).reshape(S, 2, T, F).contiguous()
        Y = torch.empty(S, T, F, 2, device=dev)
        K._chk(K._lib().se_train_mask_fwd(xm.data_ptr(), spec.data_ptr(), Y.data_ptr(), S, M, T, F, K._st()))
        pred = synthesis(g["sig"], Y, B, g["Ks"], L, g["skip"])
        model._hip_aux = (crm, _x0(spec, N, B, M, T, F))
        ctx.eng, ctx.ws, ctx.spec, ctx.xm, ctx.g, ctx.chain = eng, ws, spec, xm, g, None
        return pred

    @staticmethod
    def _forward_chains(ctx, model, eng, mixture, flags, lens):
        """Rows are the caller's outside, the engine's inside: a fresh batch is sorted by window count (FsnEngine.train_chain_order), a
        carried one keeps its slots; mixture is permuted on the way in, pred / crm / x on the way out."""
        B, M, L = mixture.shape
        dev = mixture.device
        order, idx = eng.train_chain_order(flags, lens, dev)
        if order is not None:
            mixture = mixture.index_select(0, idx)
            flags, lens = [flags[i] for i in order], [lens[i] for i in order]
        g = model._chain_geometry(mixture, flags, lens)
        N, T, F, rows = g["N"], g["T"], g["F"], g["rows"]
        S = N * B
        spec = stft_rows(g["sig"], mixture, B, M, L, rows["off0"], rows["len"], g["P"], N, T, F)
        ws = torch.empty(eng.train_ws_bytes_chains(B, L, lens, flags), dtype=torch.uint8, device=dev)
        crm = eng.train_fwd_chains(spec, B, L, lens, flags, ws, N, order, idx)    # [N, B, 2, F, T], zeros in the dead windows
        # the mask runs over all N * B segments: a dead segment has a zero spectrum (and, in the backward, a zero gradient)
        xm = crm.permute(0, 1, 2, 4, 3).reshape(S, 2, T, F).contiguous()
        Y = torch.empty(S, T, F, 2, device=dev)
        K._chk(K._lib().se_train_mask_fwd(xm.data_ptr(), spec.data_ptr(), Y.data_ptr(), S, M, T, F, K._st()))
        pred = synthesis_rows(g["sig"], Y, B, g["Ks"], L, rows["skip"], rows["len"])
        x0 = _x0(spec, N, B, M, T, F)
        if idx is not None:
            pred = torch.empty_like(pred).index_copy_(0, idx, pred)
            crm, x0 = torch.empty_like(crm).index_copy_(1, idx, crm), torch.empty_like(x0).index_copy_(1, idx, x0)
        model._hip_aux = (crm, x0)
        ctx.eng, ctx.ws, ctx.spec, ctx.xm, ctx.g, ctx.chain = eng, ws, spec, xm, g, (flags, lens, idx)
        return pred

    @staticmethod
    def backward(ctx, dpred):
        g = ctx.g
        B, M, L, N, T, F = g["B"], g["M"], g["L"], g["N"], g["T"], g["F"]
        S, dev = N * B, dpred.device
        dpred = dpred.contiguous().float()
        if ctx.chain is None:
            dY = synthesis_adjoint(g["sig"], dpred, B, N, L, g["skip"], g["Ks"], T, F)
        else:
            flags, lens, idx = ctx.chain
            if idx is not None:
                dpred = dpred.index_select(0, idx)
            dY = synthesis_adjoint_rows(g["sig"], dpred, B, N, L, g["rows"]["skip"], g["rows"]["len"], g["Ks"], T, F)
        dx = torch.empty(S, 2, T, F, device=dev)
        K._chk(K._lib().se_train_mask_bwd(dY.data_ptr(), ctx.xm.data_ptr(), ctx.spec.data_ptr(), dx.data_ptr(), S, M, T, F, g["n_fft"], K._st()))
        dcrm = dx.view(N, B, 2, T, F).permute(0, 1, 2, 4, 3).contiguous()
        grads = [torch.empty(s, device=dev) for s in ctx.shapes]
        if ctx.chain is None:
            ctx.eng.train_bwd(dcrm, B, N, ctx.ws, grads)
        else:
            ctx.eng.train_bwd_chains(dcrm, B, L, lens, flags, ctx.ws, grads)
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

    def _chain_geometry(self, mixture, flags, lens):
        """_geometry of a batch of chunk chains: per-utterance Nb / off0 / skip as host lists, and as device int64 rows for the row kernels"""
        B, M, L = mixture.shape
        n_fft, Ks = self._args["n_fft"], self.segment_length
        g = ragged_geometry(lens, flags, Ks, self._hop, n_fft)
        dev = mixture.device
        g.update(B=B, M=M, L=L, n_fft=n_fft, F=self.num_freqs, sig=_sig(dev, n_fft, self._win, self._hop, Ks),
                 rows=dict(off0=_rows(g["off0"], dev), len=_rows(g["lengths"], dev), skip=_rows(g["skip"], dev)))
        return g

    def realtime_process(self, mixture, source=None, flag=False, train=False, lengths=None):
        """flag: a bool or ONE value for the batch, or one value per utterance; lengths (optional): B ints <= Lmax, host values or a
        tensor read once, here - nothing later in the call synchronises for them.  See the module docstring for the chains contract."""
        if train:
            if lengths is not None:
                raise NotImplementedError("train=True takes one flag and one length for the whole batch")
            return super().realtime_process(mixture, source, flag, True)
        B, _, Lmax = mixture.shape
        chain = None
        if lengths is not None or (isinstance(flag, (list, tuple)) and len(flag) > 1) or (isinstance(flag, torch.Tensor) and flag.numel() > 1):
            flags, lens = _as_flags(flag, B), _as_lengths(lengths, B, Lmax)
            if len(set(flags)) == 1 and min(lens) == Lmax:
                flag = flags[0]   # a uniform batch IS the scalar call
            else:
                chain = (tuple(flags), tuple(lens))
        else:
            flag = _as_flag(flag[0] if isinstance(flag, (list, tuple)) else flag)
        if not torch.is_grad_enabled() and mixture.is_cuda:
            if chain is None:
                return super().realtime_process(mixture, source, flag, False)
            return super().realtime_process(mixture, source, list(chain[0]), False, lengths=list(chain[1]))
        self._cur_flag = flag
        if self._hip:
            pred, crm, x = self._hip_forward(mixture, flag if chain is None else chain)
            s = None if source is None else self._mic0_spec(source, flag if chain is None else chain)
        elif chain is None:
            pred, crm, x, s = self._torch_forward(mixture, source, flag)
        else:
            pred, crm, x, s = self._torch_forward_chains(mixture, source, list(chain[0]), list(chain[1]))
        if source is None:
            return pred
        return pred, crm.detach(), s.detach(), x.detach()

    # ---- kernels ----
    def _hip_forward(self, mixture, flag):
        params = list(self.parameters())
        pred = FSNFunction.apply(self, mixture, flag, *params)
        crm, x0 = self._hip_aux
        self._hip_aux = None
        return pred, crm, x0

    def _mic0_spec(self, source, flag):
        """mic 0 of the source's windows [N, B, 2, F, T]; flag: a bool, or (flags, lengths): per-row offsets, zero beyond each length"""
        src = source[:, :1].contiguous().float()
        if isinstance(flag, tuple):
            g = self._chain_geometry(src, list(flag[0]), list(flag[1]))
            sspec = stft_rows(g["sig"], src, g["B"], 1, g["L"], g["rows"]["off0"], g["rows"]["len"], g["P"], g["N"], g["T"], g["F"])
        else:
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
        # the counter is one int for the batch, or - once a chains call has run - one value per utterance [B, 1, 1, 1]
        st[key], st[key + "_step"] = rm, torch.clamp(step + 1, max=80) if isinstance(step, torch.Tensor) else min(step + 1, 80)
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

    # ---- torch restatement of a batch of chunk chains ----
    _STATE_KEYS = ("mean_fb", "mean_fb_step", "mean_sb", "mean_sb_step", "fh", "sh")

    def _chain_state(self, B, like):
        """The state of B utterances as a chains call keeps it - every entry a tensor with one row (F rows for the sub band) per utterance:
        the carried state brought to that form, or (nothing carried) the state after a reset, spelled out."""
        st, F, NL = self._tstate or {}, self.num_freqs, self._args["num_layers"]
        out = {}
        for key in ("mean_fb", "mean_sb"):
            rm, step = st.get(key), st.get(key + "_step", 0)
            out[key] = like.new_zeros(B, 1, 1, 1) if rm is None else rm
            out[key + "_step"] = step if isinstance(step, torch.Tensor) else like.new_full((B, 1, 1, 1), float(step))
        for key, rows, H in (("fh", B, self._args["fb_hidden"]), ("sh", B * F, self._args["sb_hidden"])):
            out[key] = st.get(key) or [(like.new_zeros(rows, H), like.new_zeros(rows, H)) for _ in range(NL)]
        return out

    def _merge_state(self, mask, a, b):
        """per utterance: a where mask [B] holds, else b"""
        F = self.num_freqs
        out = {}
        for key in self._STATE_KEYS:
            if key in ("fh", "sh"):
                m = (mask if key == "fh" else mask.repeat_interleave(F))[:, None]   # sub band: row b * F + f
                out[key] = [(torch.where(m, ha, hb), torch.where(m, ca, cb)) for (ha, ca), (hb, cb) in zip(a[key], b[key])]
            else:
                out[key] = torch.where(mask.view(-1, 1, 1, 1), a[key], b[key])
        return out

    def _torch_forward_chains(self, mixture, source, flags, lens):
        """B independent chunk chains in one call.  Every statistic of the model is per utterance and window positions do not depend on
        the length, so all utterances run the N = max N_b windows of the longest; state, means and counters are kept per utterance and
        an utterance's carried state is taken after its OWN last window, its output cut from its own samples."""
        B, M, Lmax = mixture.shape
        K_ = self.segment_length
        P = K_ // 2
        q = ragged_geometry(lens, flags, K_, self._hop, self._nfft)
        N, dev = q["N"], mixture.device
        carried = None
        if any(flags):
            if self._tstate is None or "fh" not in self._tstate:
                raise RuntimeError("flag=True continues a previous chunk of this path: start with flag=False")
            if self._tstate["fh"][0][0].shape[0] != B:
                raise RuntimeError(f"flag=True continues row b of the carried state, which holds {self._tstate['fh'][0][0].shape[0]} utterances, not {B}")
            carried = self._chain_state(B, mixture)
        self._tstate = None
        state = self._chain_state(B, mixture)   # after a reset
        if carried is not None:
            state = self._merge_state(torch.tensor(flags, device=dev), carried, state)

        def windows(x):   # [B, C, Lmax] -> the N windows of every utterance's own samples [B, C, N, F, T]
            xp = torch.cat([Fn.pad(x[b:b + 1, :, :lens[b]], (-q["off0"][b], (N + 1) * P + q["off0"][b] - lens[b])) for b in range(B)])
            idx = (torch.arange(N, device=dev) * P)[:, None] + torch.arange(K_, device=dev)[None, :]
            return self._stft(xp[:, :, idx])

        X = windows(mixture)
        Nb = torch.tensor(q["Nb"], device=dev)
        final, crms = state, []
        for n in range(N):
            state = dict(state)
            crms.append(self._torch_window(X[:, :, n], state))
            if n + 1 in q["Nb"]:
                final = self._merge_state(Nb == n + 1, state, final)
        self._tstate = final
        live = (torch.arange(N, device=dev)[:, None] < Nb[None, :]).to(mixture.dtype).view(N, B, 1, 1, 1)
        crm = torch.stack(crms, dim=0) * live   # [N, B, 2, F, T]: exact zeros past every utterance's own last window
        m = 9.9 * (crm >= 9.9) - 9.9 * (crm <= -9.9) + crm * (crm.abs() < 9.9)  # decompress_cIRM, utility.py:439-442
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        X0 = X[:, 0].transpose(0, 1)        # [N, B, F, T]
        re, im = X0.real, X0.imag
        Y = torch.complex(m[:, :, 0] * re - m[:, :, 1] * im, m[:, :, 1] * re + m[:, :, 0] * im)
        y = self._istft(Y).transpose(0, 1)  # [B, N, K]
        full = (y[:, 0::2].reshape(B, -1)[:, P:] + y[:, 1::2].reshape(B, -1)[:, :-P]) / 2
        pred = torch.stack([Fn.pad(full[b, q["skip"][b]:q["skip"][b] + lens[b]], (0, Lmax - lens[b])) for b in range(B)])
        x0 = torch.stack([re, im], dim=2)
        s0 = None
        if source is not None:
            S0 = windows(source[:, :1])[:, 0].transpose(0, 1)
            s0 = torch.stack([S0.real, S0.imag], dim=2)
        return pred, crm, x0, s0
