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
from .call_plan import call_plan, overlap_add_cut, windows
from .train_stages import _sig, stft, synthesis, synthesis_adjoint
from .training import _TrainableMixin

EPS = 1e-8  # fullsubnet.py:12


def _x0(spec, N, B, M, T, F):
    """mic 0 of spec [N][B*M][T][F][2] in the reference's layout [N, B, 2, F, T]"""
    return spec.view(N, B, M, T, F, 2)[:, :, 0].permute(0, 1, 4, 3, 2).contiguous()


class FSNFunction(torch.autograd.Function):
    """pred = realtime_process(mixture, flag, train=False)[0] on the kernels.  forward(ctx, model, mixture, plan, *params) with params
    in state_dict order (what fsn_train_bwd writes); plan: the call's CallPlan - uniform: fsn_train_*, chains: fsn_train_*_chains."""

    @staticmethod
    def forward(ctx, model, mixture, plan, *params):
        """Chains: rows are the caller's outside, the engine's inside - a fresh batch is sorted by window count
        (FsnEngine.train_chain_order), a carried one keeps its slots; mixture is permuted on the way in, pred / crm / x on the way out."""
        K._need_gpu(mixture, params[0])
        eng = model._engine_for(mixture)  # (re)loads the weights when an optimizer step changed them
        mixture = mixture.contiguous().float()
        B, M, L = mixture.shape
        dev = mixture.device
        if plan.uniform and plan.flag and eng._order is not None and len(eng._order) == B:
            plan = model._plan(mixture, [True] * B, uniform=False)  # the carried batch was permuted by a chains call: keep the caller's row b on its utterance
        ctx.shapes = [p.shape for p in params]
        order = idx = None
        if not plan.uniform:
            order, idx = eng.train_chain_order(plan.flags, plan.lengths, dev)
            if order is not None:
                mixture = mixture.index_select(0, idx)
                plan = model._plan(mixture, [plan.flags[i] for i in order], [plan.lengths[i] for i in order], uniform=False)
        flags, lens = plan.flags, plan.lengths
        g = model._geometry(mixture, plan)
        N, T, F = g["N"], g["T"], g["F"]
        S = N * B
        spec = stft(plan, g["sig"], mixture, M)
        if plan.uniform:
            ws = torch.empty(eng.train_ws_bytes(B, N), dtype=torch.uint8, device=dev)
            crm = eng.train_fwd(spec, B, N, plan.flag, ws)                                # [N, B, 2, F, T]
        else:
            ws = torch.empty(eng.train_ws_bytes_chains(B, L, lens, flags), dtype=torch.uint8, device=dev)
            crm = eng.train_fwd_chains(spec, B, L, lens, flags, ws, N, order, idx)    # [N, B, 2, F, T], zeros in the dead windows
        # the mask runs over all N * B segments: a dead segment has a zero spectrum (and, in the backward, a zero gradient)
        xm = crm.permute(0, 1, 2, 4, 3).reshape(S, 2, T, F).contiguous()
        Y = torch.empty(S, T, F, 2, device=dev)
        K._chk(K._lib().se_train_mask_fwd(xm.data_ptr(), spec.data_ptr(), Y.data_ptr(), S, M, T, F, K._st()))
        pred = synthesis(plan, g["sig"], Y)
        x0 = _x0(spec, N, B, M, T, F)
        if idx is not None:
            pred = torch.empty_like(pred).index_copy_(0, idx, pred)
            crm, x0 = torch.empty_like(crm).index_copy_(1, idx, crm), torch.empty_like(x0).index_copy_(1, idx, x0)
        model._hip_aux = (crm, x0)
        ctx.eng, ctx.ws, ctx.spec, ctx.xm, ctx.g, ctx.idx = eng, ws, spec, xm, g, idx
        return pred

    @staticmethod
    def backward(ctx, dpred):
        g = ctx.g
        plan = g["plan"]
        B, M, L, N, T, F = g["B"], g["M"], g["L"], g["N"], g["T"], g["F"]
        S, dev = N * B, dpred.device
        dpred = dpred.contiguous().float()
        if ctx.idx is not None:
            dpred = dpred.index_select(0, ctx.idx)
        dY = synthesis_adjoint(plan, g["sig"], dpred)
        dx = torch.empty(S, 2, T, F, device=dev)
        K._chk(K._lib().se_train_mask_bwd(dY.data_ptr(), ctx.xm.data_ptr(), ctx.spec.data_ptr(), dx.data_ptr(), S, M, T, F, g["n_fft"], K._st()))
        dcrm = dx.view(N, B, 2, T, F).permute(0, 1, 2, 4, 3).contiguous()
        grads = [torch.empty(s, device=dev) for s in ctx.shapes]
        if plan.uniform:
            ctx.eng.train_bwd(dcrm, B, N, ctx.ws, grads)
        else:
            ctx.eng.train_bwd_chains(dcrm, B, L, plan.lengths, plan.flags, ctx.ws, grads)
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

    def _plan(self, x, flag=False, lengths=None, uniform=None):
        """the CallPlan of realtime_process(x [B, C, L], flag, lengths); uniform=False: the chains form whatever the triage says"""
        return call_plan(flag, lengths, x.shape[0], x.shape[-1], self.segment_length, self._hop, self._nfft, uniform=uniform)

    def _geometry(self, mixture, plan):
        """the plan's geometry and the model's own sizes"""
        B, M, L = mixture.shape
        return dict(plan.geo, plan=plan, B=B, M=M, L=L, n_fft=self._nfft, F=self.num_freqs,
                    sig=_sig(mixture.device, self._nfft, self._win, self._hop, self.segment_length))

    def realtime_process(self, mixture, source=None, flag=False, train=False, lengths=None):
        """flag: a bool or ONE value for the batch, or one value per utterance; lengths (optional): B ints <= Lmax, host values or a
        tensor read once, here - nothing later in the call synchronises for them.  See the module docstring for the chains contract."""
        if train:
            if lengths is not None:
                raise NotImplementedError("train=True takes one flag and one length for the whole batch")
            return super().realtime_process(mixture, source, flag, True)
        plan = self._plan(mixture, flag, lengths)
        if not torch.is_grad_enabled() and mixture.is_cuda:
            if plan.uniform:
                return super().realtime_process(mixture, source, plan.flag, False)
            return super().realtime_process(mixture, source, plan.flags, False, lengths=plan.lengths)
        if self._hip:
            pred, crm, x = self._hip_forward(mixture, plan)
            s = None if source is None else self._mic0_spec(source, plan)
        elif plan.uniform:
            pred, crm, x, s = self._torch_forward(mixture, source, plan)
        else:
            pred, crm, x, s = self._torch_forward_chains(mixture, source, plan)
        if source is None:
            return pred
        return pred, crm.detach(), s.detach(), x.detach()

    # ---- kernels ----
    def _hip_forward(self, mixture, plan):
        params = list(self.parameters())
        pred = FSNFunction.apply(self, mixture, plan, *params)
        crm, x0 = self._hip_aux
        self._hip_aux = None
        return pred, crm, x0

    def _mic0_spec(self, source, plan):
        """mic 0 of the source's windows [N, B, 2, F, T], by the mixture's plan: per-row offsets, zero beyond each length"""
        src = source[:, :1].contiguous().float()
        sspec = stft(plan, _sig(src.device, self._nfft, self._win, self._hop, self.segment_length), src, 1)   # [N, B, T, F, 2]
        return sspec.permute(0, 1, 4, 3, 2).contiguous()

    # ---- torch restatement (the checker) ----
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

    def _torch_outputs(self, plan, X, crm, source):
        """What both restatement loops end with: crm [N, B, 2, F, T] over the windows' spectra X [B, M, N, F, T] -> decompress_cIRM
        (utility.py:439-442), complex multiply with mic 0, iSTFT, overlap-add.  -> (pred, crm, x0, s0: mic 0 of mixture / source)"""
        m = 9.9 * (crm >= 9.9) - 9.9 * (crm <= -9.9) + crm * (crm.abs() < 9.9)
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        X0 = X[:, 0].transpose(0, 1)        # [N, B, F, T]
        re, im = X0.real, X0.imag
        Y = torch.complex(m[:, :, 0] * re - m[:, :, 1] * im, m[:, :, 1] * re + m[:, :, 0] * im)
        pred = overlap_add_cut(plan, self._istft(Y).transpose(0, 1))  # [B, N, K] -> [B, L]
        s0 = None
        if source is not None:
            S0 = self._stft(windows(plan, source[:, :1]))[:, 0].transpose(0, 1)
            s0 = torch.stack([S0.real, S0.imag], dim=2)
        return pred, crm, torch.stack([re, im], dim=2), s0

    def _torch_forward(self, mixture, source, plan):
        """The uniform call: one state for the batch, the CumLayerNorm step counters Python ints (_torch_forward_chains keeps them as
        float32 tensors per utterance, which rounds the running-mean ratio differently: the two loops stay apart)."""
        if not plan.flag:
            self._tstate = {}
        elif self._tstate is None:
            raise RuntimeError("flag=True continues a previous chunk of this path: start with flag=False")
        X = self._stft(windows(plan, mixture))   # [B, M, N, F, T]
        st = self._tstate
        crm = torch.stack([self._torch_window(X[:, :, n], st) for n in range(plan.N)], dim=0)   # [N, B, 2, F, T]
        return self._torch_outputs(plan, X, crm, source)

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

    def _torch_forward_chains(self, mixture, source, plan):
        """B independent chunk chains in one call.  Every statistic of the model is per utterance and window positions do not depend on
        the length, so all utterances run the N = max N_b windows of the longest; state, means and counters are kept per utterance and
        an utterance's carried state is taken after its OWN last window, its output cut from its own samples."""
        B, N, dev = plan.B, plan.N, mixture.device
        carried = None
        if plan.any_flag:
            if self._tstate is None or "fh" not in self._tstate:
                raise RuntimeError("flag=True continues a previous chunk of this path: start with flag=False")
            if self._tstate["fh"][0][0].shape[0] != B:
                raise RuntimeError(f"flag=True continues row b of the carried state, which holds {self._tstate['fh'][0][0].shape[0]} utterances, not {B}")
            carried = self._chain_state(B, mixture)
        self._tstate = None
        state = self._chain_state(B, mixture)   # after a reset
        if carried is not None:
            state = self._merge_state(torch.tensor(plan.flags, device=dev), carried, state)
        X = self._stft(windows(plan, mixture))   # the N windows of every utterance's own samples [B, M, N, F, T]
        Nb = torch.tensor(plan.Nb, device=dev)
        final, crms = state, []
        for n in range(N):
            state = dict(state)
            crms.append(self._torch_window(X[:, :, n], state))
            if n + 1 in plan.Nb:
                final = self._merge_state(Nb == n + 1, state, final)
        self._tstate = final
        live = (torch.arange(N, device=dev)[:, None] < Nb[None, :]).to(mixture.dtype).view(N, B, 1, 1, 1)
        crm = torch.stack(crms, dim=0) * live   # [N, B, 2, F, T]: exact zeros past every utterance's own last window
        return self._torch_outputs(plan, X, crm, source)
