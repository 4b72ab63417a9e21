"""Drop-in `Generator` and `Hifi_GAN` (reference Hifi-GAN/hifigan.py:444-656 and 884-896; predict.py builds `Hifi_GAN` from config.yaml
and calls it): the CRN-shaped U-Net of the GAN line of work - weight-normed convolutions with the self-gate tanh(y) * sigmoid(y) and no
norm, an LSTM bottleneck with a running-mean norm, and a postnet of twelve 1x1 convolutions at 128 channels on every bin.

Same constructors, state_dict keys and shapes (`*.weight_g` / `*.weight_v`, the `net.0.*` aliases), same entry points:

    Generator.forward(x[B, M, F, T, 2], post=True) -> (y, y_before) [B, F, T, 2]    one window, stateful; post=False: (y, None)
    Generator.realtime_process(mixture[B, M, L], post=True, reset=False) -> (pred, pred_before) [B, L]
    Generator.realtime_process_chains(mixture[B, M, Lmax], resets, lengths=None, post=True) -> (pred, pred_before) [B, Lmax]
    Generator.reset(), reset_norm(streams=None), use_hip_kernels(flag), kernel_geometry_error(), max_segments, _last_path, _last_passes, taps
    Generator.use_hip_training(flag, chains=False), hip_training_error()
    Hifi_GAN.forward(x, post=True) = generator.realtime_process(x, reset=False, post=post)[0]
    Hifi_GAN.train_stage(x, y, stage=1, y_hat=None, y_before=None, reset=True) -> loss (stages 1 and 2)
    Hifi_GAN.realtime_process_chains(x, resets, lengths=None, post=True) = the generator's, its first result
    Hifi_GAN.train_stage_chains(x, y, resets, lengths, stage=2, y_hat=None, y_before=None) -> loss, the mean over the streams

Quirks of the reference that are kept:
  * `reset=True` prepends half a window of zeros, resets and strips the half window (the `flag=False` of the other models);
    `reset=False` continues whatever is carried, and starts from zero buffers WITHOUT the half window on a fresh model.
  * The bottleneck norm (GlobalLayerNorm(last=True, time=True), hifigan.py:306-349) subtracts a running mean and has no variance:
    alpha = step / (step + D), g = alpha * g_old + (1 - alpha) * mean(window), step += D, where D is the FEATURE width x.shape[-1]
    (13 * C_last), not the frame count.  SequenceModel.reset() never resets it, so (mean, step) SURVIVE reset(): the third utterance
    of a session is normalised by a mean that began with the first.  `reset_norm()` is this project's addition for a truly fresh model.
    The mean is [B]; a batch size other than the carried one is refused with ValueError, except a carried batch of 1, which the
    reference's broadcast spreads over the new batch (the other direction breaks its reshape).
  * `realtime_process(post=False)` raises TypeError, as the reference does (it assigns None into a tensor, hifigan.py:634).
  * `Hifi_GAN` holds the generator only: `discriminator.*` checkpoint keys are dropped on load, and there is no remove_weight_norm
    (the reference's calls a method that does not exist).

`realtime_process_chains` serves B independent callers in one call (chunk chains, call_plan.py; `resets[b]` = not `flag[b]`): stream b is
mixture[b, :, :lengths[b]], resets or continues row b of the carried state on its own, and leaves what it would carry alone.  The norm's
quirk is kept PER STREAM: resets[b] does not touch mean[b] or stream b's step count, and streams that advance by different window counts
have different counts - `_nstate["step"]` is one int while they are all equal and a list of B ints (host values, from the plan) once they
are not; reset_norm(streams=[b]) zeroes one stream's pair, for a slot handed to a new caller.  The restatement runs every stream literally
alone; the kernel path runs every pass on the prefix of streams still running (streaming.StreamingMixin._prefix_passes), the LSTM and
the norm's scan stopping at each stream's own last window (se_hifi_lstm_rows, se_hifi_seqnorm_rows).  Resets and lengths all alike are
the uniform call - `realtime_process`, which still takes ONE `reset`.

Three paths (the choice, the refusals and the carried state are streaming.StreamingMixin's; `reset` = not `flag`):
  * the torch restatement (CPU, grad enabled, training mode, or after use_hip_kernels(False)): plain torch ops, differentiable.
    Encoder, decoder and postnet run every window of a pass at once (the conv history of window n is the tail of window n - 1's
    input); the LSTM - its cell written out, h and c detached at every window seam as the reference does - and the norm's scan are
    sequential.  `forward` is the same code on one window.
  * the kernel path (`realtime_process` of a GPU tensor, eval mode, grad disabled): train_stages.py's signal chain, the convolutions
    on se_train_conv_w and the dense layers on se_train_gemm with the weight norm folded on the host (g * v / ||v|| in float64),
    everything else on csrc/se_hifi.hip.  An unsupported geometry raises ValueError naming the limit; there is no fallback.
  * HIP training (opt-in, `use_hip_training(True)`; `hip_training_error()` names what it does not cover): `realtime_process` of a GPU
    tensor with grad enabled is ONE autograd node, hifigan_training.HifiFunction - the kernel path's forward as it stands (bit-equal
    outputs and carried state, `_last_path` "kernel") and a backward on the same kernels plus csrc/se_hifi_train.hip.  Uniform calls
    only, unless `use_hip_training(True, chains=True)`: then realtime_process_chains, and a uniform call on per-stream norm step
    counts, are one node as well - its forward the inference chains path, its backward the sum over the streams of each one alone.
`Hifi_GAN.train_stage(x, y, stage)` is the reference's training loss on losses.stft_loss for stages 1 and 2 (no discriminators: 3 raises);
`train_stage_chains(x, y, resets, lengths, stage)` is the mean over the streams of that loss on every stream's own samples.
Carried state: the encoder levels' last input window, the LSTM's (h, c) per layer - `_tstate` / `_kstate` - and the norm's
(mean [B], step) in `_nstate`, which both paths share because nothing but reset_norm() ends it.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn
from torch import nn

from . import train_ops as K
from .call_plan import as_flags, istft_windows, overlap_add_cut, segment_geometry, windows
from .streaming import StreamingMixin
from .train_stages import _ip, _new, _p, _rows, _run, gru_steps, input_features, istft_into, own_last_slab, stft

EPS = 1e-8
POST_CHANNELS = 128
POST_LAYERS = 12


def fold_weight_norm(g, v):
    """torch.nn.utils.weight_norm's weight, g * v / ||v|| with the norm over every dim but 0, in float64.  dim 0 of a ConvTranspose2d
    weight is the INPUT channel."""
    v, g = v.detach().double(), g.detach().double()
    return v * (g / v.flatten(1).norm(dim=1).reshape(g.shape))


def _w(m):
    """the weight of a weight-normed holder, differentiable"""
    v = m.weight_v
    return v * (m.weight_g / v.flatten(1).norm(dim=1).reshape(m.weight_g.shape))


def _weight_normed(m):
    """A conv / linear module as torch.nn.utils.weight_norm leaves it - parameters bias, weight_g, weight_v in that order - without the
    forward hook: the module only owns the parameters, the restatement calls the functional forms with `_w`."""
    w = m.weight.detach()
    del m._parameters["weight"]
    m.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).reshape(-1, *([1] * (w.dim() - 1))))
    m.weight_v = nn.Parameter(w.clone())
    return m


def _gate(y):
    return torch.tanh(y) * torch.sigmoid(y)


class _Conv(nn.Module):  # TemporalConv2d, hifigan.py:193-247
    def __init__(self, cin, cout, kernel, stride, dil, padding, dropout):
        super().__init__()
        self.padding = padding[1]
        self.conv = _weight_normed(nn.Conv2d(cin, cout, kernel, stride=stride, padding=(padding[0], 0), dilation=(1, dil)))
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)


class _Deconv(nn.Module):  # TemporalConvTranspose2d, hifigan.py:250-302: no residualnorm
    def __init__(self, cin, cout, k, dil, dropout):
        super().__init__()
        self.padding = (k - 1) * dil
        self.conv = _weight_normed(nn.ConvTranspose2d(cin, cout, (5, k), stride=(2, 1), padding=(2, 0), dilation=(1, dil)))
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)
        self.residualmask = _weight_normed(nn.Conv2d(cout, cout, (1, 1)))
        self.residual = _weight_normed(nn.Conv2d(cout, cout, (1, 1)))


class _MeanNorm(nn.Module):  # GlobalLayerNorm(last=True, time=True): the affine only, the running mean lives in Generator._nstate
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(1, 1, 1, dim))
        self.bias = nn.Parameter(torch.zeros(1, 1, 1, dim))


class _Seq(nn.Module):  # SequenceModel(sequence_model="LSTM", output_activate_function="Tanh"), hifigan.py:351-441
    def __init__(self, dim, hidden, num_layers):
        super().__init__()
        self.sequence_model = nn.LSTM(input_size=dim, hidden_size=hidden, num_layers=num_layers, batch_first=True)
        self.fc_output_layer = _weight_normed(nn.Linear(hidden, dim))
        self.norm = _MeanNorm(dim)


def _lstm(x, m, hc):
    """nn.LSTM (batch_first) written out: x [B, T, In], hc = [(h, c) per layer] -> (out [B, T, H], [(h, c) per layer])"""
    H = m.hidden_size
    new = []
    for l in range(m.num_layers):
        gi = x @ getattr(m, f"weight_ih_l{l}").t() + (getattr(m, f"bias_ih_l{l}") + getattr(m, f"bias_hh_l{l}"))
        w_hh = getattr(m, f"weight_hh_l{l}")
        h, c = hc[l]
        outs = []
        for t in range(x.shape[1]):
            g = gi[:, t] + h @ w_hh.t()
            c = torch.sigmoid(g[:, H:2 * H]) * c + torch.sigmoid(g[:, :H]) * torch.tanh(g[:, 2 * H:3 * H])
            h = torch.sigmoid(g[:, 3 * H:]) * torch.tanh(c)
            outs.append(h)
        x = torch.stack(outs, dim=1)
        new.append((h, c))
    return x, new


class Generator(StreamingMixin, nn.Module):
    def __init__(self, num_channels, num_freqs, hidden, segment_length, num_layers=1, num_inputs=3, kernel_size=3, dropout=0.0,
                 sample_rate=16000, win_length=25, hop_length=10, n_fft=400):
        super().__init__()
        self.segment_length = segment_length
        self.num_freqs = num_freqs
        self._cfg = dict(num_channels=list(num_channels), hidden=hidden, num_layers=num_layers, num_inputs=num_inputs, kernel_size=kernel_size,
                         n_fft=n_fft)
        # _tstate: dict(buf=[[B, C, F, P] per level], hc=[(h, c) per layer]); _kstate: dict(B, buf=[[B][C][T][F] per level], h=[..], c=[..]);
        # _nstate: None or dict(mean [B], step int), shared by both paths; taps: enc / seq / dec / post of every forward
        self._init_streaming(num_inputs, sample_rate, win_length, hop_length)
        self._nstate = None
        self._last_passes = None   # kernel path: the passes of the last call, [(first window, windows, streams), ...]
        self._hip_train = False
        self._hip_train_chains = False
        L = len(num_channels)
        convs, deconvs = [], []
        for i in range(L):
            cin = (2 * num_inputs - 1) if i == 0 else num_channels[i - 1]
            convs.append(_Conv(cin, num_channels[i], (5, kernel_size), (2, 1), 2 ** i, (2, (kernel_size - 1) * 2 ** i), dropout))
            deconvs.insert(0, _Deconv(num_channels[i], 2 if i == 0 else cin, kernel_size, 2 ** (L - i - 1), dropout))
        self.convlist = nn.ModuleList(convs)
        self.deconvlist = nn.ModuleList(deconvs)
        self.gru = _Seq((num_freqs // 16 + 1) * num_channels[-1], hidden, num_layers)
        chans = [2] + [POST_CHANNELS] * (POST_LAYERS - 1) + [2]
        self.postnet = nn.ModuleList([_Conv(chans[i], chans[i + 1], (1, 1), (1, 1), 1, (0, 0), 0.0) for i in range(POST_LAYERS)])

    # ---- reference contract ------------------------------------------------------------------------------------------------
    def reset_norm(self, streams=None):
        """Forget the bottleneck norm's running mean and step count, which reset() keeps as the reference does.  streams: the rows to
        forget (their mean and step become 0, which normalises the row's next window by its own mean as a fresh model does - the slot
        of a caller that left, handed to the next); None: all of it.  Nothing carried: nothing to do."""
        ns = self._nstate
        if streams is None or ns is None:
            self._nstate = None if streams is None else ns
            return
        B = ns["mean"].shape[0]
        rows = sorted({int(b) for b in (streams.reshape(-1).tolist() if torch.is_tensor(streams) else streams)})
        if rows and not 0 <= rows[0] <= rows[-1] < B:
            raise ValueError(f"reset_norm(streams={rows}): the running mean is carried for streams 0 .. {B - 1}")
        mean, steps = ns["mean"].clone(), self._steps_of(ns, B)
        for b in rows:
            mean[b], steps[b] = 0.0, 0
        self._nstate = self._norm_state(mean, steps)

    def forward(self, x, post=True):
        """One window [B, M, F, T, 2] -> (y, y_before) on the torch restatement, carrying the encoder buffers, (h, c) and the running mean."""
        ns = self._norm_for(x.shape[0])
        if ns is not None and isinstance(ns["step"], list):
            raise ValueError("forward() runs the batch through one norm step count, and the streams' counts differ after a chunk-chain "
                             "call: use realtime_process, or reset_norm()")
        (Y, Yb), self._tstate, self._nstate = self._pass(x[:, :, None], self._tstate, ns, post)
        return Y[:, 0], (Yb[:, 0] if post else None)

    def realtime_process(self, mixture, post=True, reset=False):
        """-> (pred, pred_before) [B, L]; reset is ONE value for the batch: the uniform call of realtime_process_chains."""
        if isinstance(reset, (list, tuple)) or (torch.is_tensor(reset) and reset.numel() != 1):
            raise ValueError("Generator.realtime_process takes one `reset` for the whole batch: per-utterance resets and lengths (chunk "
                             "chains) are realtime_process_chains(mixture, resets, lengths)")
        return self.realtime_process_chains(mixture, reset, None, post)

    def realtime_process_chains(self, mixture, resets, lengths=None, post=True):
        """mixture [B, M, Lmax] -> (pred, pred_before) [B, Lmax]: B independent streams.  resets: a bool, one value or B values;
        lengths: None or B values in [1, Lmax].  Stream b is mixture[b, :, :lengths[b]] whatever the padding holds; where resets[b] it
        starts from zero buffers and zero (h, c) behind the reference's half window of zeros, elsewhere it continues row b of the
        carried state; both outputs are zero at [b, lengths[b]:], and the carried state afterwards holds, per stream, what the stream
        alone would carry - its running mean and its own norm step count included, which resets[b] does not touch.  Resets and
        lengths all alike: the uniform call, which is realtime_process."""
        if not post:
            raise TypeError("realtime_process(post=False): the reference cannot either - forward returns None for the result before the "
                            "postnet and realtime_process assigns it into a tensor (hifigan.py:634); use forward(x, post=False)")
        B, M, L = mixture.shape
        self._norm_for(B)
        plan = self._plan([not r for r in as_flags(resets, B)], lengths, B, L, M)
        return getattr(self, f"_{self._admit(mixture, plan)}_call")(mixture, plan)

    # ---- HIP training (hifigan_training.HifiFunction) ------------------------------------------------------------------------------
    def use_hip_training(self, flag=True, chains=False):
        """True: realtime_process of a GPU tensor with grad enabled runs forward AND backward on the kernels, as ONE autograd node
        (hifigan_training.HifiFunction) that returns (pred, pred_before), sharing the carried state with the inference kernel path.
        False (default): grad-enabled calls take the restatement.  Raises ValueError at once for a geometry or a dropout setting the
        training kernels do not cover.  chains=False (default): uniform calls on one carried norm step count only, anything else is
        refused; chains=True: realtime_process_chains (per-stream resets and lengths) and a uniform call that finds per-stream norm
        step counts are one HifiFunction node too - forward = the inference chains path, backward = the sum over the streams of what
        each, run alone, would give every parameter."""
        if flag:
            err = self.hip_training_error()
            if err:
                raise ValueError(f"Generator HIP training: {err}")
        self._hip_train = bool(flag)
        self._hip_train_chains = bool(flag) and bool(chains)
        return self

    def hip_training_error(self):
        """None when HifiFunction can train this model as it stands, else the limit that fails (geometry, or active dropout)."""
        err = self.kernel_geometry_error()
        if err:
            return err
        if self.training and any(b.dropout.p > 0 for b in list(self.convlist) + list(self.deconvlist) + list(self.postnet)):
            return "dropout is active in training mode: the training kernels have no dropout (use the restatement, or dropout = 0)"
        return None

    def _choose_path(self, mixture):
        if self._hip_train and mixture.is_cuda and torch.is_grad_enabled():
            return "train"
        return super()._choose_path(mixture)

    def _train_call(self, mixture, plan):
        from .hifigan_training import HifiFunction
        err = self.hip_training_error()
        if err:
            raise ValueError(f"Generator HIP training: {err}")
        ns = self._norm_for(mixture.shape[0])
        if not self._hip_train_chains and (not plan.uniform or (ns is not None and isinstance(ns["step"], list))):
            raise ValueError("Generator HIP training runs uniform calls only (one reset, full lengths, one carried norm step count): "
                             "per-stream resets, lengths or step counts train on the restatement, use_hip_training(False)")
        K._need_gpu(mixture, self.gru.norm.weight)
        if mixture.shape[1] != self._mics:
            raise ValueError(f"Generator HIP training: {mixture.shape[1]} microphones, the model is built for {self._mics}")
        return HifiFunction.apply(self, mixture, plan, *[p for _, p in self.named_parameters()])

    def _norm_for(self, B):
        """the carried (mean, step) for a batch of B; refuses another batch size, except the carried batch of 1 the reference broadcasts"""
        ns = self._nstate
        if ns is not None and ns["mean"].shape[0] not in (1, B):
            raise ValueError(f"the bottleneck norm's running mean is carried for a batch of {ns['mean'].shape[0]} utterances, got {B}: "
                             "reset() keeps it as the reference does, reset_norm() forgets it")
        return ns

    @staticmethod
    def _steps_of(ns, B):
        """the norm's step count per stream: B ints, whatever form is carried"""
        step = 0 if ns is None else ns["step"]
        return list(step) if isinstance(step, list) else [step] * B

    @staticmethod
    def _norm_state(mean, step):
        """`_nstate`: step stays ONE int while every stream's count is the same (a uniform call on such a state keeps it so), else a
        list of B ints - host values, known from the plan's window counts"""
        return dict(mean=mean, step=step[0] if isinstance(step, list) and len(set(step)) == 1 else step)

    @staticmethod
    def _batch_of(state):
        return state["buf"][0].shape[0]

    # ---- torch restatement ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _mask_apply(m, noisy):
        """m [S, 2, F, T], noisy [S, F, T, 2] (microphone 0) -> [S, F, T, 2]: decompress_cIRM, complex product"""
        m = 9.9 * (m >= 9.9) - 9.9 * (m <= -9.9) + m * (torch.abs(m) < 9.9)
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        return torch.stack([m[:, 0] * noisy[..., 0] - m[:, 1] * noisy[..., 1], m[:, 1] * noisy[..., 0] + m[:, 0] * noisy[..., 1]], dim=-1)

    def _pass(self, X, st, ns, post=True):
        """X [B, M, N, F, T, 2], N windows in order -> ((Y, Y_before) [B, N, F, T, 2], state, norm state), all out of place.  N > 1
        needs every encoder history shorter than a window."""
        B, M, N, F, T, _ = X.shape
        taps = self.taps
        x = X.transpose(1, 2).reshape(B * N, M, F, T, 2)
        noisy = x[:, 0]
        re, im = x[..., 0], x[..., 1]
        ang = torch.arctan(im / (re + EPS) + EPS)
        h = torch.cat([torch.sqrt(re ** 2 + im ** 2 + 1e-10), ang[:, :1] - ang[:, 1:]], dim=1)
        residuals, bufs = [h], []
        for i, blk in enumerate(self.convlist):
            P, (C_, F_) = blk.padding, h.shape[1:3]
            buf = st["buf"][i] if st is not None else h.new_zeros(B, C_, F_, P)
            if N == 1:
                prev = buf
            else:   # the history of window n: the last P frames of window n - 1's input (P < T), detached as the reference's buffer is
                prev = torch.cat([buf[:, None], h.reshape(B, N, C_, F_, T)[:, :-1, ..., T - P:].detach()], dim=1).reshape(B * N, C_, F_, P)
            inp = torch.cat([prev, h], dim=-1)
            bufs.append(inp.reshape(B, N, C_, F_, P + T)[:, -1, ..., -P:].detach())
            h = _gate(blk.dropout(Fn.conv2d(inp, _w(blk.conv), blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=blk.conv.dilation)))
            residuals.append(h)
        if taps is not None:
            taps["enc"] = h
        # bottleneck: LSTM over the windows in order (h, c detached at every seam), fc + tanh, running-mean norm
        Cl, Fl = h.shape[1:3]
        D = Cl * Fl
        seq = h.reshape(B, N, D, T).transpose(2, 3)                    # [B, N, T, D]
        g = self.gru
        hc = st["hc"] if st is not None else [(seq.new_zeros(B, g.sequence_model.hidden_size),) * 2 for _ in range(g.sequence_model.num_layers)]
        outs = []
        for n in range(N):
            o, hc = _lstm(seq[:, n], g.sequence_model, hc)
            hc = [(a.detach(), b.detach()) for a, b in hc]
            outs.append(o)
        o = torch.tanh(torch.stack(outs, dim=1) @ _w(g.fc_output_layer).t() + g.fc_output_layer.bias)   # [B, N, T, D]
        means = o.mean(dim=(2, 3))
        gm, step = (None, 0) if ns is None else (ns["mean"].to(means), ns["step"])
        gs = []
        for n in range(N):
            if gm is None:
                cur = means[:, n]
            else:
                alpha = step / (step + D)
                cur = alpha * gm + (1.0 - alpha) * means[:, n]
            gs.append(cur)
            gm, step = cur.detach(), step + D
        o = (o - torch.stack(gs, dim=1)[:, :, None, None]) * g.norm.weight + g.norm.bias
        h = o.transpose(2, 3).reshape(B * N, Cl, Fl, T)
        if taps is not None:
            taps["seq"] = h.reshape(B * N, D, T)
        L = len(self.deconvlist)
        for j, blk in enumerate(self.deconvlist):
            y = Fn.conv_transpose2d(h, _w(blk.conv), blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=blk.conv.dilation)
            y = _gate(blk.dropout(y)[..., -T:])
            if j < L - 1:
                res = residuals[-2 - j]
                if res.shape[2] > y.shape[2]:
                    y = Fn.pad(y, (0, 0, 0, res.shape[2] - y.shape[2]))
                elif res.shape[2] < y.shape[2]:
                    y = y[:, :, :res.shape[2]]
                m = torch.sigmoid(Fn.conv2d(res, _w(blk.residualmask), blk.residualmask.bias))
                y = m * torch.tanh(Fn.conv2d(res, _w(blk.residual), blk.residual.bias)) + (1.0 - m) * y
            h = y
        if taps is not None:
            taps["dec"] = h
        Yb = None
        if post:
            Yb = self._mask_apply(h, noisy).reshape(B, N, F, T, 2)
            for blk in self.postnet:
                h = _gate(blk.dropout(Fn.conv2d(h, _w(blk.conv), blk.conv.bias)))
            if taps is not None:
                taps["post"] = h
        Y = self._mask_apply(h, noisy).reshape(B, N, F, T, 2)
        return (Y, Yb), dict(buf=bufs, hc=hc), dict(mean=gm, step=step)

    def _restate(self, mixture, plan, st, ns):
        """One uniform call on the restatement, out of place -> ((pred, pred_before) [B, L], state, norm state)"""
        X = self.spectrum(windows(plan, mixture))
        step = max(1, int(self.max_segments)) if all(b.padding < X.shape[4] for b in self.convlist) else 1
        Ys, Ybs = [], []
        for n0 in range(0, X.shape[2], step):
            (Y, Yb), st, ns = self._pass(X[:, :, n0:n0 + step], st, ns)
            Ys.append(Y)
            Ybs.append(Yb)
        c = self._cfg
        preds = [overlap_add_cut(plan, istft_windows(torch.view_as_complex(torch.cat(v, dim=1).contiguous()), c["n_fft"], self._hop, self._win, mixture.dtype))
                 for v in (Ys, Ybs)]
        return preds, st, ns

    @staticmethod
    def _state_row(st, b, B):
        return dict(buf=[t[b:b + 1] for t in st["buf"]], hc=[(h[b:b + 1], c[b:b + 1]) for h, c in st["hc"]])

    @staticmethod
    def _state_merge(rows):
        return dict(buf=[torch.cat(ts) for ts in zip(*(r["buf"] for r in rows))],
                    hc=[tuple(torch.cat(v) for v in zip(*layer)) for layer in zip(*(r["hc"] for r in rows))])

    def _torch_call(self, mixture, plan):
        """Uniform, on ONE carried norm step count: the batch as it stands.  Chains (the oracle of the kernel path), and a uniform call
        on per-stream step counts: every stream literally alone, as streaming.StreamingMixin._torch_call runs them - B = 1, its own
        length and reset, its own row of `_tstate` - and with its own (mean[b], step[b]), which the mixin's form has no place for, as
        it has none for the second result; the outputs padded to the batch width, the states merged row by row."""
        B, M, Lmax = mixture.shape
        st, ns = self._tstate, self._norm_for(B)
        if plan.uniform and not (ns is not None and isinstance(ns["step"], list)):
            preds, st, ns = self._restate(mixture, plan, st if plan.flag else None, ns)
        else:
            steps, alone = self._steps_of(ns, B), []
            for b, (f, L) in enumerate(zip(plan.flags, plan.lengths)):
                own = None if ns is None else dict(mean=ns["mean"][b:b + 1] if ns["mean"].shape[0] > 1 else ns["mean"], step=steps[b])
                alone.append(self._restate(mixture[b:b + 1, :, :L], self._plan(f, None, 1, L, M), self._state_row(st, b, B) if f and st is not None else None, own))
            preds = [torch.cat([Fn.pad(a[0][i], (0, Lmax - L)) for a, L in zip(alone, plan.lengths)]) for i in range(2)]
            st = self._state_merge([a[1] for a in alone])
            ns = self._norm_state(torch.cat([a[2]["mean"] for a in alone]), [a[2]["step"] for a in alone])
        self._tstate, self._nstate = st, ns
        return preds[0], preds[1]

    # ---- kernel path ---------------------------------------------------------------------------------------------------------
    def _plan_channels(self, M):
        return [2 * M - 1] + self._cfg["num_channels"]

    def kernel_geometry_error(self):
        """None when the kernel path supports this geometry, else the limit that fails (realtime_process raises it as ValueError)."""
        c = self._cfg
        M, k, H, ch = c["num_inputs"], c["kernel_size"], c["hidden"], [2 * c["num_inputs"] - 1] + c["num_channels"]
        Lv = len(c["num_channels"])
        geo = segment_geometry(0, False, self.segment_length, self._hop, c["n_fft"], ch)
        T, F0, Fq = geo["T"], geo["F0"], geo["Fq"]
        D = (self.num_freqs // 16 + 1) * ch[-1]
        if M != 3:
            return f"num_inputs = {M}: the feature and mask kernels are built for 3 microphones"
        if k != 3:
            return f"kernel_size = {k}: the convolution kernels are 5 x 3"
        if F0 != self.num_freqs:
            return f"STFT gives n_fft / 2 + 1 = {F0} frequencies, the model is built for num_freqs = {self.num_freqs}"
        if (k - 1) * 2 ** (Lv - 1) >= T:
            return f"encoder history (k - 1) * 2^(L - 1) = {(k - 1) * 2 ** (Lv - 1)} frames is not shorter than the {T}-frame window"
        for i in range(Lv):
            if (ch[i + 1] + 31) // 32 * 32 not in (32, 64, 128):
                return f"convlist.{i}: {ch[i + 1]} output channels do not pad to 32, 64 or 128 (the conv kernels' GEMM rows)"
        if H % 8 or H > 1024:
            return f"hidden = {H}: a multiple of 8 (the GEMM's inner dimension) up to 1024 (the LSTM step keeps 8 rows of h in LDS)"
        if Fq[Lv] * ch[-1] != D:
            return f"the encoder leaves {Fq[Lv]} x {ch[-1]} features, the LSTM is built for {D}"
        if D % 8:
            return f"{D} bottleneck features: the GEMM's inner dimension must be a multiple of 8"
        for j in range(Lv - 1):
            kk = Lv - 1 - j
            if Fq[kk] < 2 * Fq[kk + 1] - 1:
                return f"deconvlist.{j}: {2 * Fq[kk + 1] - 1} frequencies do not fit the {Fq[kk]}-bin skip tensor"
        if 2 * Fq[1] - 1 != self.num_freqs:
            return f"last decoder block gives {2 * Fq[1] - 1} frequencies, num_freqs = {self.num_freqs}"
        return None

    def _folded(self, name, m):
        """the folded fp32 weight of a weight-normed module, once per parameter version"""
        return self._cached(("w", name), [m.weight_g, m.weight_v], lambda: fold_weight_norm(m.weight_g, m.weight_v).float().contiguous())

    def _postnet_pack(self):
        """every postnet weight (folded, [Co][Ci]) and bias in one buffer, in layer order: what se_hifi_postnet reads"""
        ps = [p for blk in self.postnet for p in (blk.conv.weight_g, blk.conv.weight_v, blk.conv.bias)]
        return self._cached("postnet", ps, lambda: torch.cat([t.reshape(-1) for blk in self.postnet for t in (
            fold_weight_norm(blk.conv.weight_g, blk.conv.weight_v).float(), blk.conv.bias.detach().float())]).contiguous())

    def _lstm_bias(self, l):
        m = self.gru.sequence_model
        bi, bh = getattr(m, f"bias_ih_l{l}"), getattr(m, f"bias_hh_l{l}")
        return self._cached(("lstm_b", l), [bi, bh], lambda: (bi.detach().float() + bh.detach().float()).contiguous())

    def _kernel_pass(self, mixture, plan, sig, state, n0, Nc, ysegs, start, sv=None):
        """Windows [n0, n0 + Nc) of the call: STFT, features, encoder, bottleneck, decoder, both masks and the postnet, iSTFT into
        ysegs; advances `state` (a dict this call owns: buf, h, c and the norm's mean [B]).  Chunk chains: `plan` holds the streams
        of this pass (the leading plan.B rows of mixture and of every state tensor; ysegs may be wider); a stream runs the LSTM and
        the norm's scan over its own windows of the pass only, and its encoder buffers stop at its own last window.  start: the
        norm's step count per caller row as the call found it.  A stream that has a window at n0 has run exactly n0 windows of this
        call, so it enters the pass at start[row] + n0 * D: one count for all takes the scalar kernel, else se_hifi_seqnorm_rows.
        sv (a dict): the pass re-run for hifigan_training's backward - the LSTM also stores its gates and cells (se_hifi_lstm_train_fwd,
        chains: se_hifi_lstm_train_fwd_rows; the same arithmetic), sv receives every activation the backward reads and, where the norm
        took its `_rows` form, the per-stream step table and live counts, and the pass stops after the decoder: no mask, no postnet,
        nothing written to ysegs."""
        lib, st, dev = K._lib(), K._st, mixture.device
        c = self._cfg
        B, M, T, F0, ch, Fq, H, NL, Lv = plan.B, mixture.shape[1], plan.T, plan.F0, plan.ch, plan.Fq, c["hidden"], c["num_layers"], len(self.convlist)
        S, TT = Nc * B, Nc * T
        keep = sv is not None
        ypre, xs, lstm, dec = [], [], [], []
        steps, live = gru_steps(plan, dev, T, 1, n0, Nc)   # chains: per stream its LSTM steps and its own windows of this pass
        spec = stft(plan, sig, mixture, M, n0, Nc)
        # encoder: xin[i] = [Nc + 1][B][C][T][F], slab 0 = the carried input window of level i (its time history)
        xin = []
        for i in range(Lv):
            t_ = _new(Nc + 1, B, ch[i], T, Fq[i], dev=dev)
            t_[0].copy_(state["buf"][i])
            xin.append(t_)
        input_features(spec, xin[0], S, B, M, ch[0], T, F0)
        for i, blk in enumerate(self.convlist):
            Ci, Co, Fi, Fo = ch[i], ch[i + 1], Fq[i], Fq[i + 1]
            y = _new(S, Co, T, Fo, dev=dev)
            K.conv_w(0, _p(xin[i], B * Ci * T * Fi), _p(xin[i]), self._folded(("conv", i), blk.conv), Ci * 15, 15, blk.conv.bias, y, S, Ci, Co, T, Fi, Fo, 2 ** i)
            if i < Lv - 1:
                dst = _p(xin[i + 1], B * Co * T * Fo)
            else:
                enc = _new(S, Co, T, Fo, dev=dev)
                dst = _p(enc)
            _run("k_hifi_gate", 0.0, lib.se_hifi_gate, _p(y), dst, y.numel(), st())
            if keep:
                ypre.append(y)
        del y
        # bottleneck
        Cl, Fl = ch[Lv], Fq[Lv]
        D = Cl * Fl
        x_l = _new(B * TT, D, dev=dev)
        _run("k_hifi_rows", 0.0, lib.se_hifi_rows, _p(enc), _p(x_l), Nc, B, Cl, T, Fl, st())
        del enc
        m = self.gru.sequence_model
        for l in range(NL):
            gi = K._gemm(x_l, getattr(m, f"weight_ih_l{l}"), self._lstm_bias(l))
            out, hT, cT = _new(B * TT, H, dev=dev), _new(B, H, dev=dev), _new(B, H, dev=dev)
            args = (_p(gi), _p(state["h"][l]), _p(state["c"][l]), _p(getattr(m, f"weight_hh_l{l}")), _p(out), _p(hT), _p(cT))
            if keep:
                gates, cs = _new(B * TT, 4 * H, dev=dev), _new(B * TT, H, dev=dev)
                if steps is None:
                    _run("k_hifi_lstm_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm_train_fwd, *args, _p(gates), _p(cs), B, TT, H, st())
                else:
                    _run("k_hifi_lstm_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm_train_fwd_rows, *args, _p(gates), _p(cs), _ip(steps), B, TT, H, st())
                xs.append(x_l)
                lstm.append(dict(gates=gates, cs=cs, out=out, h0=state["h"][l], c0=state["c"][l]))
            elif steps is None:
                _run("k_hifi_lstm_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm, *args, B, TT, H, st())
            else:
                _run("k_hifi_lstm_step", 2.0 * B * 4 * H * H * TT, lib.se_hifi_lstm_rows, *args, _ip(steps), B, TT, H, st())
            state["h"][l], state["c"][l] = hT, cT
            x_l = out
            del gi
        fc = self.gru.fc_output_layer
        o = K._gemm(x_l, self._folded("fc", fc), fc.bias)           # [B][Nc T][D], before the tanh
        del x_l, out
        mean_in, step = state["mean"], [start[b] + n0 * D for b in plan.rows]
        mean_out, wm = _new(B, dev=dev), _new(B * Nc, dev=dev)
        h = _new(S, Cl, T, Fl, dev=dev)
        nm = self.gru.norm
        step_dev = cnt = None
        if plan.uniform and len(set(step)) == 1:
            _run("k_hifi_seqnorm", 0.0, lib.se_hifi_seqnorm, _p(o), _p(nm.weight), _p(nm.bias), _p(mean_in), float(step[0]), _p(wm), _p(mean_out), _p(h),
                 Nc, B, Cl, T, Fl, st())
        else:
            step_dev, cnt = _rows(step, dev), (live if live is not None else _rows(plan.live(n0, Nc), dev))
            _run("k_hifi_seqnorm", 0.0, lib.se_hifi_seqnorm_rows, _p(o), _p(nm.weight), _p(nm.bias), _p(mean_in), _ip(step_dev), _ip(cnt), _p(wm),
                 _p(mean_out), _p(h), Nc, B, Cl, T, Fl, st())
        state["mean"] = mean_out
        if keep:
            # rows: the pass took the `_rows` norm (per-stream step table and live counts, device int64 [B]); else one step for all
            sv.update(spec=spec, xin=xin, ypre=ypre, xs=xs, lstm=lstm, o=o, wm=wm, step=float(step[0]), dec=dec, rows=step_dev is not None,
                      step_rows=step_dev, cnt=cnt)
        del o
        # decoder
        Ci, Fi = Cl, Fl
        for j, blk in enumerate(self.deconvlist):
            Co, Fy = blk.conv.weight_v.shape[1], 2 * Fi - 1
            w = self._folded(("deconv", j), blk.conv)
            yd = _new(S, Co, T, Fy, dev=dev)
            if keep:   # the level's input, transposed-convolution output and (below) 1x1 pair: what its backward reads
                dec.append(dict(x_in=h, yd=yd, Ci=Ci, Co=Co, Fi=Fi, Fy=Fy))
            for kind in (1, 2):
                K.conv_w(kind, _p(h), None, w, 15, Co * 15, blk.conv.bias, yd, S, Ci, Co, T, Fi, Fy, 2 ** j)
            if j < Lv - 1:
                k = Lv - 1 - j
                Cr, Fr = ch[k], Fq[k]
                if Fr < Fy or Cr != Co:
                    raise RuntimeError("decoder / skip geometry outside the reference's (the crop branch of hifigan.py:294 is never taken)")
                res = _p(xin[k], B * Cr * T * Fr)
                uv = _new(S, 2 * Co, T, Fr, dev=dev)   # residual | residualmask
                K.conv_w(3, res, None, self._folded(("res", j), blk.residual), Cr, 1, blk.residual.bias, uv, S, Cr, Co, T, Fr, Fr, 0, 0, 2 * Co, 0)
                K.conv_w(3, res, None, self._folded(("resmask", j), blk.residualmask), Cr, 1, blk.residualmask.bias, uv, S, Cr, Co, T, Fr, Fr, 0, 0, 2 * Co, Co)
                h = _new(S, Co, T, Fr, dev=dev)
                _run("k_hifi_skip", 0.0, lib.se_hifi_skip, _p(yd), _p(uv), _p(h), S, Co, T, Fy, Fr, st())
                if keep:
                    dec[-1].update(uv=uv, k=k, Cr=Cr, Fr=Fr)
                del uv
                Ci, Fi = Co, Fr
            else:
                h = _new(S, Co, T, Fy, dev=dev)
                _run("k_hifi_gate", 0.0, lib.se_hifi_gate, _p(yd), _p(h), yd.numel(), st())
        del yd
        if keep:
            sv["hdec"] = h
            return
        Y = _new(S, T, F0, 2, dev=dev)
        _run("k_tmask", 0.0, lib.se_train_mask_fwd, _p(h), _p(spec), _p(Y), S, M, T, F0, st())
        istft_into(plan, sig, Y, ysegs[1], n0, Nc)
        hp = _new(S, 2, T, F0, dev=dev)
        _run("k_hifi_postnet", 2.0 * S * T * F0 * (2 * 2 * POST_CHANNELS + (POST_LAYERS - 2) * POST_CHANNELS * POST_CHANNELS), lib.se_hifi_postnet,
             _p(h), _p(self._postnet_pack()), _p(hp), S, T, F0, st())
        _run("k_tmask", 0.0, lib.se_train_mask_fwd, _p(hp), _p(spec), _p(Y), S, M, T, F0, st())
        istft_into(plan, sig, Y, ysegs[0], n0, Nc)
        # every stream's own last window of the pass; slab 0 (what it carried) where it has none
        state["buf"] = [own_last_slab(plan, xin[i], live, copy=True) for i in range(Lv)]

    @torch.no_grad()
    def _kernel_process(self, mixture, plan, record=None):
        """One call on the kernels, uniform or chains: StreamingMixin._prefix_passes' schedule over `_kernel_pass`, the running mean as
        the entry of the working state that no reset clears.  The norm's step counts never travel with it: they follow from the plan.
        record (a list; HifiFunction): receives, per pass, (the pass's plan, sig, the state it entered with, n0, Nc, start, the pass's
        mixture rows - the sorted prefix mix[:Bp], a view) - the state's tensors are replaced, never written, so holding them keeps
        the entry state."""
        dev, B = mixture.device, mixture.shape[0]
        c = self._cfg
        H, NL, Lv, T, ch, Fq = c["hidden"], c["num_layers"], len(self.convlist), plan.T, plan.ch, plan.Fq
        old = self._kstate if plan.any_flag else None
        ns = self._norm_for(B)
        mean = torch.zeros(B, device=dev) if ns is None else ns["mean"].to(device=dev, dtype=torch.float32).expand(B).contiguous()
        start = self._steps_of(ns, B)

        def fresh(B):
            return dict(buf=[torch.zeros(B, ch[i], T, Fq[i], device=dev) for i in range(Lv)],
                        h=[torch.zeros(B, H, device=dev) for _ in range(NL)], c=[torch.zeros(B, H, device=dev) for _ in range(NL)], mean=mean)
        carried = None if old is None else dict(buf=old["buf"], h=old["h"], c=old["c"], mean=mean)
        def run_pass(mix, sub, sig, state, n0, Nc, ysegs):
            if record is not None:
                record.append((sub, sig, {k: list(v) if isinstance(v, list) else v for k, v in state.items()}, n0, Nc, start, mix))
            self._kernel_pass(mix, sub, sig, state, n0, Nc, ysegs, start)
        preds, new, passes = self._prefix_passes(mixture, plan, carried, fresh, 2, run_pass, unflagged=("mean",))
        self._kstate = dict(B=B, buf=new["buf"], h=new["h"], c=new["c"])
        self._nstate = self._norm_state(new["mean"], [s + n * ch[Lv] * Fq[Lv] for s, n in zip(start, plan.Nb)])
        self._last_passes = passes
        return preds[0], preds[1]


class Hifi_GAN(nn.Module):
    """The reference's wrapper (hifigan.py:884-896) with the generator only: `nffts` / `n_mels` configure its discriminators, which are
    not built here, and `discriminator.*` checkpoint keys are dropped on load (predict.py loads with strict=False)."""

    def __init__(self, nffts, n_mels, num_channels, num_freqs, hidden, segment_length, num_layers=1, num_inputs=3, kernel_size=3, dropout=0.0,
                 sample_rate=16000, win_length=25, hop_length=10, n_fft=400):
        super().__init__()
        self.generator = Generator(num_channels, num_freqs, hidden, segment_length, num_layers, num_inputs, kernel_size, dropout, sample_rate,
                                   win_length, hop_length, n_fft)

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("discriminator.")}, strict=strict, **kw)

    def forward(self, x, post=True):
        y, _ = self.generator.realtime_process(x, reset=False, post=post)
        return y

    def realtime_process_chains(self, x, resets, lengths=None, post=True):
        """the generator's realtime_process_chains, its first result (this project's addition: the reference serves one stream)"""
        return self.generator.realtime_process_chains(x, resets, lengths, post)[0]

    def train_stage(self, x, y, stage=1, y_hat=None, y_before=None, reset=True):
        """The reference's training loss (hifigan.py:917-956) without its print.  Stage 2: 0.5 * stft_loss(y_hat, y, phase=True) +
        0.5 * stft_loss(y_before, y, phase=True), (y_hat, y_before) = generator.realtime_process(x, reset=reset) unless y_hat is
        given.  Stage 1 asks the generator for post=False, which raises TypeError here as it fails in the reference; with y_hat given
        it is stft_loss(y_hat, y, phase=True).  Stage 3 needs the discriminators, which are not built: NotImplementedError."""
        from .losses import stft_loss
        if stage not in (1, 2):
            raise NotImplementedError(f"train_stage(stage={stage}): the adversarial stage needs the discriminators, which are not built here "
                                      "(stages 1 and 2 train the generator on stft_loss)")
        if y_hat is None:
            y_hat, y_before = self.generator.realtime_process(x, reset=reset, post=stage != 1)
        if stage == 1:
            return stft_loss(y_hat, y, phase=True)
        return 0.5 * stft_loss(y_hat, y, phase=True) + 0.5 * stft_loss(y_before, y, phase=True)

    def train_stage_chains(self, x, y, resets, lengths, stage=2, y_hat=None, y_before=None):
        """train_stage for a batch of chunk chains (this project's addition): x [B, M, Lmax], y [B, Lmax], stream b being its first
        lengths[b] samples, resets[b] as realtime_process_chains takes them.  -> the MEAN OVER THE STREAMS of the reference's loss
        of every stream alone: stft_loss(y_hat[b:b+1, :lengths[b]], y[b:b+1, :lengths[b]], phase=True), stage 2 the 0.5 / 0.5 pair with
        y_before.  That is the "every caller alone" rule applied to the loss, and deliberately NOT the reference's whole-batch form:
        stft_loss divides Frobenius norms taken over the whole batch, which would weigh a stream by its neighbours' energy and read
        the padding.  (y_hat, y_before) = generator.realtime_process_chains(x, resets, lengths) unless y_hat is given.  Stage 1
        without y_hat raises TypeError and stage 3 NotImplementedError, as train_stage does.  Plain torch on losses.stft_loss."""
        from .call_plan import as_lengths
        from .losses import stft_loss
        if stage not in (1, 2):
            raise NotImplementedError(f"train_stage_chains(stage={stage}): the adversarial stage needs the discriminators, which are not built "
                                      "here (stages 1 and 2 train the generator on stft_loss)")
        if y_hat is None:
            y_hat, y_before = self.generator.realtime_process_chains(x, resets, lengths, post=stage != 1)
        lens = as_lengths(lengths, y.shape[0], y.shape[-1])
        total = 0.0
        for b, L in enumerate(lens):
            one = stft_loss(y_hat[b:b + 1, :L], y[b:b + 1, :L], phase=True)
            if stage == 2:
                one = 0.5 * one + 0.5 * stft_loss(y_before[b:b + 1, :L], y[b:b + 1, :L], phase=True)
            total = total + one
        return total / len(lens)
