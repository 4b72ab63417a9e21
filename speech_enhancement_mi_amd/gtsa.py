"""Drop-in `GTSA` (reference GTSA.py:247-407, byte-identical to GTSA_original.py, which train.py / predict.py import): a transformer
whose keys and values live in a rolling buffer of `maxlen` frames carried across the 3200-sample windows, with the score function

    softmax(|Q K^T * G / sqrt(model_dim)|) V,   G[i, j] = exp(-(i - j)^2 / (delta^2 + 1e-8)),   delta learned.

Same constructor (the ignored `num_heads` / `model_dim` included), state_dict keys and shapes (`layers.i.attention.ind`, the
`last_conv.net.0.*` aliases), same entry points:

    forward(x[B, M, F, T, 2]) -> [B, F, T, 2]          one window, stateful (GTSA.py:277-307)
    realtime_process(mixture[B, M, L], flag=False, lengths=None) -> [B, L]   GTSA.py:370-407; per-utterance flags / lengths: chunk chains
    reset(), use_hip_kernels(flag), kernel_geometry_error(), max_segments, _last_path, _last_passes

Within one layer, attention at window n reads keys and values of windows <= n of that layer's INPUT, never an attention output of the
same layer: a layer has no sequential dependence across windows, so a call runs layer by layer with every window at once.  The rolling
buffer is a TAPE per (sequence, head): the carried buffer in rows [0, maxlen), the projected keys / values of the call's N windows after
it; window n attends to rows [(n + 1) T, (n + 1) T + maxlen) - the reference's cat([bk[:, T:], k]) applied n + 1 times - and the call
leaves the last maxlen rows behind.  The two-frame input buffer of `last_conv` is the previous window's last two input frames.

Two paths (the call's contract, the choice between them, the refusals and the carried state: streaming.StreamingMixin, shared with
general_beamformer.GeneralBeamformer):
  * the torch restatement (CPU, grad enabled, training mode, or after use_hip_kernels(False)): plain torch ops, differentiable.
    `realtime_process` uses the tape, `forward` the reference's window-by-window form, both on the same state.
  * the kernel path (`realtime_process` of a GPU tensor, grad disabled, eval mode): STFT / iSTFT / overlap-add of train_stages.py, the
    nn.Linear layers of the even layers and the three convolutions of `last_conv` on se_train_gemm, everything else on
    csrc/se_gtsa.hip.  An unsupported geometry raises ValueError naming the limit; there is no fallback.

A call with per-utterance flags or lengths is a batch of B independent CHUNK CHAINS (call_plan.py): utterance b runs its own Nb[b] windows
and leaves the state it would carry alone.  The restatement runs every utterance literally alone (streaming.py's `_torch_call`); the kernel
path runs every pass on the prefix of streams still running (streaming.py's `_prefix_passes`), the tape tail and the last_conv buffer
stopping at each stream's own last window (se_gtsa_tape_rows, se_gtsa_lastframes_rows).
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as Fn
from torch import nn

from . import train_ops as K
from .call_plan import chain_passes  # noqa: F401  (re-exported: the schedule was first written here)
from .streaming import StreamingMixin
from .train_stages import _ip, _new, _p, _rows, _run, istft_into, stft

EPS = 1e-8


class _Norm(nn.Module):  # GlobalLayerNorm(time=False), GTSA.py:74-129: denominator sqrt(var + 1e-10) + 1e-8
    def __init__(self, dim, last=False):
        super().__init__()
        shape = (1, 1, dim) if last else (1, dim, 1)
        self.weight = nn.Parameter(torch.ones(shape))
        self.bias = nn.Parameter(torch.zeros(shape))
        self.last = last


def _gln(x, norm):
    """x [..., A, B'] with statistics over the last two dims; affine over the last dim (last=True) or the one before it."""
    mean = x.mean((-2, -1), keepdim=True)
    var = ((x - mean) ** 2).mean((-2, -1), keepdim=True)
    return (x - mean) / (torch.sqrt(var + 1e-10) + EPS) * norm.weight + norm.bias


class _Attention(nn.Module):  # MutiheadAttention, GTSA.py:139-203
    def __init__(self, num_heads, model_dim, maxlen):
        super().__init__()
        self.num_heads, self.model_dim, self.maxlen = num_heads, model_dim, maxlen
        self.ql = nn.Linear(model_dim, model_dim)
        self.kl = nn.Linear(model_dim, model_dim)
        self.vl = nn.Linear(model_dim, model_dim)
        self.linear = nn.Linear(model_dim, model_dim)
        self.delta = nn.Parameter(torch.ones(1))
        ind = torch.arange(1, maxlen + 1).unsqueeze(1).repeat(1, maxlen)
        self.register_buffer("ind", -(ind - ind.transpose(0, 1)) ** 2)

    def gauss(self, T):
        """the query rows of G: [T, maxlen]"""
        return torch.exp(self.ind[-T:] / (self.delta ** 2 + EPS))

    def split(self, z):
        """[Bs, R, dim] -> [heads * Bs, R, D], head-major as the reference's cat(split(.), dim=0)"""
        return torch.cat(torch.split(z, self.model_dim // self.num_heads, dim=-1), dim=0) if self.num_heads > 1 else z

    def merge(self, z, Bs):
        return torch.cat(torch.split(z, Bs, dim=0), dim=-1) if self.num_heads > 1 else z

    def fresh(self, x, Bs):
        return x.new_zeros(Bs * self.num_heads, self.maxlen, self.model_dim // self.num_heads)

    def window(self, x, bk, bv):
        """One window, the reference's form: x [Bs, T, dim] -> (out, bk, bv)"""
        Bs, T, _ = x.shape
        q, k, v = self.split(self.ql(x)), self.split(self.kl(x)), self.split(self.vl(x))
        k = torch.cat([bk[:, T:], k], dim=1)
        v = torch.cat([bv[:, T:], v], dim=1)
        s = torch.abs(torch.matmul(q, k.transpose(1, 2)) * self.gauss(T).unsqueeze(0) / math.sqrt(self.model_dim))
        o = torch.matmul(torch.softmax(s, dim=-1), v)
        return self.linear(self.merge(o, Bs)), k.detach(), v.detach()

    def tape(self, x, bk, bv):
        """N windows at once over the tape: x [Bs, N, T, dim] -> (out [Bs, N, T, dim], bk, bv)"""
        Bs, N, T, dim = x.shape
        maxlen = self.maxlen
        flat = x.reshape(Bs, N * T, dim)
        q = self.split(self.ql(flat)).reshape(-1, N, T, dim // self.num_heads)
        tk = torch.cat([bk, self.split(self.kl(flat))], dim=1)   # [heads * Bs, maxlen + N T, D]
        tv = torch.cat([bv, self.split(self.vl(flat))], dim=1)
        kw = tk.unfold(1, maxlen, T)[:, 1:]                      # window n = rows [(n + 1) T, (n + 1) T + maxlen): [.., N, D, maxlen]
        vw = tv.unfold(1, maxlen, T)[:, 1:]
        s = torch.abs(torch.matmul(q, kw) * self.gauss(T) / math.sqrt(self.model_dim))
        o = torch.matmul(torch.softmax(s, dim=-1), vw.transpose(-1, -2))   # [heads * Bs, N, T, D]
        o = self.merge(o.reshape(-1, N * T, dim // self.num_heads), Bs)
        return self.linear(o).reshape(Bs, N, T, dim), tk[:, -maxlen:].detach(), tv[:, -maxlen:].detach()


class _Layer(nn.Module):  # TransformerLayer, GTSA.py:206-242
    def __init__(self, num_heads, model_dim, fn_dim, maxlen, dropout):
        super().__init__()
        self.attention = _Attention(num_heads, model_dim, maxlen)
        self.norm_a = _Norm(model_dim, last=True)
        self.linear_in = nn.Linear(model_dim, fn_dim)
        self.linear_out = nn.Linear(fn_dim, model_dim)
        self.norm_i = _Norm(model_dim, last=True)
        self.dropout = nn.Dropout(dropout)

    def after_attention(self, a, x):
        x = _gln(a + x, self.norm_a)
        return _gln(self.linear_out(self.dropout(torch.relu(self.linear_in(x)))) + x, self.norm_i)


class _LastConv(nn.Module):  # TemporalConv1d(activation=None), GTSA.py:11-72
    def __init__(self, cin, cout, dropout):
        super().__init__()
        self.padding = 2
        self.conv = nn.Conv1d(cin, cout, 3)
        self.conv_trans = nn.Conv1d(cout, cout, 1)
        self.conv_gated = nn.Conv1d(cout, cout, 1)
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)
        self.norm = _Norm(cout)

    def gate(self, inp):
        out = self.net(inp)
        return self.conv_trans(out) * torch.sigmoid(self.conv_gated(out))


class GTSA(StreamingMixin, nn.Module):
    def __init__(self, num_mics, num_freqs, segment_length, num_layers, num_heads, model_dim, fn_dim, maxlen=500, dropout=0.0,
                 sample_rate=16000, win_length=25, hop_length=10, n_fft=400):
        super().__init__()
        self.segment_length = segment_length
        self.num_freqs = num_freqs
        self._cfg = dict(num_mics=num_mics, num_layers=num_layers, fn_dim=fn_dim, maxlen=maxlen, dropout=dropout, n_fft=n_fft)
        self._init_streaming(num_mics, sample_rate, win_length, hop_length)
        # _tstate: dict(bk=[...], bv=[...] per layer [heads * Bs, maxlen, D], buf [B, C F, 2]); _kstate: dict(B, k=[...], v=[...] per
        # layer [(b U + u) Hh + h][maxlen][D], buf [B][C][2][Fs]); taps: feat / att0 / layer1 / last of every forward
        C_ = 2 * num_mics - 1
        # num_heads / model_dim are accepted and ignored, as in the reference (GTSA.py:268-272)
        self.last_conv = _LastConv(num_freqs * C_, num_freqs * 2, dropout)
        self.layers = nn.ModuleList([_Layer(3, num_freqs, fn_dim, maxlen, dropout) if i % 2 == 0 else _Layer(1, C_, fn_dim, maxlen, dropout)
                                     for i in range(num_layers)])
        self._last_passes = None   # kernel path: the passes of the last call, [(first window, windows, streams), ...]

    # ---- reference contract ------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, **kw):
        """Checkpoints the reference saved after a run carry the rolling buffers (`layers.i.attention.bk` / `.bv`): dropped."""
        sd = {k: v for k, v in state_dict.items() if not k.endswith((".attention.bk", ".attention.bv"))}
        return super().load_state_dict(sd, strict=strict, **kw)

    def compute_loss(self, source, pred_source, length):
        """(loss, mae, sisnr), loss = 0.7 * pesq_loss + 0.3 * (-SI-SNR) (GTSA.py:411-433), on CPU or GPU tensors; a NaN loss turns all
        three into zeros without a gradient.  Inputs of fewer than 20 spectrogram frames (4864 samples) raise NotImplementedError:
        the reference's pesq_loss has no value for them (losses.pesq_loss)."""
        from .losses import gtsa_compute_loss
        return gtsa_compute_loss(source, pred_source, length)

    # ---- torch restatement ---------------------------------------------------------------------------------------------------
    @staticmethod
    def features(x):
        """x [..., M, F, T, 2] -> [..., 2M - 1, F, T] (GTSA.py:279-284)"""
        ang = torch.atan2(x[..., 1], x[..., 0])
        mag = torch.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2 + 1e-10)
        return torch.cat([mag, ang[..., :1, :, :] - ang[..., 1:, :, :]], dim=-3)

    @staticmethod
    def _mask_apply(mask, noisy):
        """mask [..., 2F, T], noisy [..., F, T, 2] (microphone 0) -> [..., F, T, 2]: decompress_cIRM, complex product"""
        F = noisy.shape[-3]
        m = torch.stack([mask[..., :F, :], mask[..., F:, :]], dim=-1)
        m = 9.9 * (m >= 9.9) - 9.9 * (m <= -9.9) + m * (torch.abs(m) < 9.9)
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        return torch.stack([m[..., 0] * noisy[..., 0] - m[..., 1] * noisy[..., 1], m[..., 1] * noisy[..., 0] + m[..., 0] * noisy[..., 1]], dim=-1)

    def _fresh_state(self, x, B):
        C_, F = 2 * self._cfg["num_mics"] - 1, self.num_freqs
        seqs = [B * C_ if i % 2 == 0 else B * F for i in range(len(self.layers))]
        return dict(bk=[l.attention.fresh(x, n) for l, n in zip(self.layers, seqs)], bv=[l.attention.fresh(x, n) for l, n in zip(self.layers, seqs)],
                    buf=x.new_zeros(B, C_ * F, 2))

    def forward(self, x):
        """One window [B, M, F, T, 2] -> [B, F, T, 2], the reference's window-by-window form on the carried state."""
        B, M, F, T, _ = x.shape
        st = self._tstate if self._tstate is not None else self._fresh_state(x[..., 0], B)
        taps = self.taps
        h = self.features(x)
        C_ = h.shape[1]
        if taps is not None:
            taps["feat"] = h.reshape(B * C_, F, T)   # as layer 0 receives it
        h = h.reshape(B, C_ * F, T)
        bk, bv = [], []
        for i, layer in enumerate(self.layers):
            h = h.reshape(B * C_, F, T) if i % 2 == 0 else h.reshape(B, C_, F, T).transpose(1, 2).reshape(B * F, C_, T)
            s = h.transpose(1, 2)
            a, k, v = layer.attention.window(s, st["bk"][i], st["bv"][i])
            bk.append(k)
            bv.append(v)
            if taps is not None and i == 0:
                taps["att0"] = a
            h = layer.after_attention(a, s).transpose(1, 2)
            if taps is not None and i == 1:
                taps["layer1"] = h   # [B F, C, T], the layer's own output layout
            h = h.reshape(B, C_ * F, T) if i % 2 == 0 else h.reshape(B, F, C_, T).transpose(1, 2).reshape(B, C_ * F, T)
        lc = self.last_conv
        m = _gln(lc.gate(torch.cat([st["buf"], h], dim=-1)), lc.norm)
        if taps is not None:
            taps["last"] = m
        buf = h[..., -2:].detach() if T > 2 else torch.cat([st["buf"], h.detach()], dim=-1)[..., -2:]
        self._tstate = dict(bk=bk, bv=bv, buf=buf)
        return self._mask_apply(m, x[:, 0])

    def _tape_pass(self, X, st):
        """X [B, M, N, F, T, 2] (N windows) -> ([B, N, F, T, 2], state): every window of the pass at once, layer by layer."""
        B, M, N, F, T, _ = X.shape
        h = self.features(X.transpose(1, 2))          # [B, N, C, F, T]
        C_ = h.shape[2]
        h = h.transpose(-1, -2)                       # [B, N, C, T, F]
        bk, bv = [], []
        for i, layer in enumerate(self.layers):
            if i % 2 == 0:
                s = h.permute(0, 2, 1, 3, 4).reshape(B * C_, N, T, F)
            else:
                s = h.permute(0, 4, 1, 3, 2).reshape(B * F, N, T, C_)
            a, k, v = layer.attention.tape(s, st["bk"][i], st["bv"][i])
            bk.append(k)
            bv.append(v)
            s = layer.after_attention(a, s)
            h = s.reshape(B, C_, N, T, F).permute(0, 2, 1, 3, 4) if i % 2 == 0 else s.reshape(B, F, N, T, C_).permute(0, 2, 4, 3, 1)
        lc = self.last_conv
        z = h.permute(0, 2, 4, 1, 3).reshape(B, C_ * F, N * T)
        inp = torch.cat([st["buf"], z], dim=-1)
        g = lc.gate(inp).reshape(B, 2 * F, N, T).transpose(1, 2)   # [B, N, 2F, T]: the norm is per window
        m = _gln(g, lc.norm)
        Y = self._mask_apply(m, X[:, 0])
        return Y, dict(bk=bk, bv=bv, buf=inp[..., -2:].detach())

    def _torch_windows(self, X, st):
        """tape passes of max_segments windows"""
        st = st if st is not None else self._fresh_state(X[..., 0, 0, 0], X.shape[0])
        outs = []
        step = max(1, int(self.max_segments))
        for n0 in range(0, X.shape[2], step):
            Y, st = self._tape_pass(X[:, :, n0:n0 + step], st)
            outs.append(Y)
        return torch.cat(outs, dim=1), st

    def _heads(self):
        return [l.attention.num_heads for l in self.layers]

    def _state_row(self, st, b, B):
        """bk / bv are head-major, [heads * B * U, maxlen, D] with row h (B U) + b U + u, so utterance b is [:, b] of [heads, B, U, ..]"""
        return dict(buf=st["buf"][b:b + 1], **{k: [t.reshape(h, B, -1, *t.shape[1:])[:, b].reshape(-1, *t.shape[1:])
                                                   for t, h in zip(st[k], self._heads())] for k in ("bk", "bv")})

    def _state_merge(self, rows):
        return dict(buf=torch.cat([r["buf"] for r in rows]),
                    **{k: [torch.cat([r[k][i].reshape(h, 1, -1, *r[k][i].shape[1:]) for r in rows], dim=1).flatten(0, 2)
                           for i, h in enumerate(self._heads())] for k in ("bk", "bv")})

    @staticmethod
    def _batch_of(state):
        return state["buf"].shape[0]

    # ---- kernel path ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _limits():
        v = [C.c_int(0) for _ in range(3)]
        K._lib().se_gtsa_limits(*(C.byref(x) for x in v))
        return tuple(x.value for x in v)

    def kernel_geometry_error(self):
        """None when the kernel path supports this geometry, else the limit that fails (realtime_process raises it as ValueError)."""
        c = self._cfg
        F, n_fft, maxlen, fn = self.num_freqs, c["n_fft"], c["maxlen"], c["fn_dim"]
        T = self.segment_length // self._hop + 1
        max_t, max_len, max_norm = self._limits()
        if c["num_mics"] != 3:
            return f"num_mics = {c['num_mics']}: the odd-layer kernels are built for 2 * 3 - 1 = 5 features per bin"
        if F != n_fft // 2 + 1:
            return f"STFT gives {n_fft // 2 + 1} frequencies, the model is built for num_freqs = {F}"
        if F % 3 or F // 3 != 67:
            return f"num_freqs = {F}: the even layers have 3 heads of num_freqs / 3, and the attention kernel is built for heads of 67 (num_freqs = 201)"
        if T > maxlen:
            return f"{T} frames per window exceed maxlen = {maxlen}: a window would reach before the carried part of the tape"
        if T > max_t or T < 3:
            return f"{T} frames per window: the kernels take 3 to {max_t}"
        if maxlen > max_len:
            return f"maxlen = {maxlen}: at most {max_len} (-(i - j)^2 exact in fp32)"
        if T * F > max_norm:
            return f"{T} x {F} values per even-layer sequence: the norm kernel holds at most {max_norm}"
        if fn % 8:
            return f"fn_dim = {fn}: the GEMM's inner dimension must be a multiple of 8"
        return None

    def _weights(self, Fs):
        """GEMM operands: K padded to Fs per F-row, q / k / v stacked, the k = 3 convolution as [2F padded to 8][3 * 5 * Fs]"""
        F = self.num_freqs
        out = []
        for i in range(0, len(self.layers), 2):
            l, a = self.layers[i], self.layers[i].attention
            ps = [a.ql.weight, a.kl.weight, a.vl.weight, a.ql.bias, a.kl.bias, a.vl.bias, a.linear.weight, l.linear_in.weight]
            out.append(self._cached(("even", i), ps, lambda a=a, l=l: dict(
                wqkv=Fn.pad(torch.cat([a.ql.weight, a.kl.weight, a.vl.weight]), (0, Fs - F)).contiguous(),
                bqkv=torch.cat([a.ql.bias, a.kl.bias, a.vl.bias]).contiguous(),
                wo=Fn.pad(a.linear.weight, (0, Fs - F)).contiguous(), win=Fn.pad(l.linear_in.weight, (0, Fs - F)).contiguous())))
        lc = self.last_conv
        Co = 2 * F
        Cp = (Co + 7) // 8 * 8

        def conv():
            w = lc.conv.weight.reshape(Co, 5, F, 3).permute(0, 3, 1, 2)          # [o][k][c][f]
            w = Fn.pad(w, (0, Fs - F)).reshape(Co, 15 * Fs)
            w2 = torch.cat([lc.conv_trans.weight.reshape(Co, Co), lc.conv_gated.weight.reshape(Co, Co)])
            return dict(w1=Fn.pad(w, (0, 0, 0, Cp - Co)).contiguous(), b1=Fn.pad(lc.conv.bias, (0, Cp - Co)).contiguous(),
                        w2=Fn.pad(w2, (0, Cp - Co)).contiguous(), b2=torch.cat([lc.conv_trans.bias, lc.conv_gated.bias]).contiguous())
        return out, self._cached("conv", [lc.conv.weight, lc.conv.bias, lc.conv_trans.weight, lc.conv_trans.bias, lc.conv_gated.weight, lc.conv_gated.bias], conv)

    def _seq_shape(self, i):
        """(U sequences per utterance, heads, head width) of layer i"""
        return (5, 3, self.num_freqs // 3) if i % 2 == 0 else (self.num_freqs, 1, 5)

    def _kernel_pass(self, mixture, plan, sig, state, n0, Nc, ysegs):
        """Windows [n0, n0 + Nc) of the call: STFT, features, the layers, the output stage, iSTFT into ysegs[0]; advances `state`.
        Chunk chains: `plan` holds the streams of this pass (the leading plan.B rows of mixture and of every state tensor; the window
        buffer may be wider), and the state stops at every stream's own last window of the pass."""
        lib, st, dev = K._lib(), K._st, mixture.device
        B, M, T, F, maxlen, fn = plan.B, mixture.shape[1], plan.T, plan.F0, self._cfg["maxlen"], self._cfg["fn_dim"]
        Fs = (F + 7) // 8 * 8
        S = Nc * B
        rows = S * 5 * T
        even_w, conv_w = self._weights(Fs)
        cnt = None if plan.uniform else _rows(plan.live(n0, Nc), dev)   # per stream: its own windows among the Nc of this pass

        def tape(kn, vn, kc, vc, ko, vo, ldk, U, Hh, D):
            if cnt is None:
                _run("k_gtsa_tape", 0.0, lib.se_gtsa_tape, kn, vn, _p(kc), _p(vc), _p(ko), _p(vo), ldk, Nc, B, U, Hh, D, T, maxlen, st())
            else:
                _run("k_gtsa_tape", 0.0, lib.se_gtsa_tape_rows, kn, vn, _p(kc), _p(vc), _p(ko), _p(vo), _ip(cnt), ldk, Nc, B, U, Hh, D, T, maxlen, st())
        spec = stft(plan, sig, mixture, M, n0, Nc)
        x = _new(S, 5, T, Fs, dev=dev)
        _run("k_gtsa_feat", 0.0, lib.se_gtsa_feat, _p(spec), _p(x), S, M, T, F, Fs, st())
        att = torch.zeros(rows, Fs, device=dev)   # even layers write columns < F only: the GEMM reads the pad as zeros
        for i, layer in enumerate(self.layers):
            a = layer.attention
            U, Hh, D = self._seq_shape(i)
            kc, vc = state["k"][i], state["v"][i]
            ko, vo = torch.empty_like(kc), torch.empty_like(vc)
            if i % 2 == 0:
                w = even_w[i // 2]
                qkv = K._gemm(x.view(rows, Fs), w["wqkv"], w["bqkv"])     # [rows][3F]
                kn, vn, ldk = _p(qkv, F), _p(qkv, 2 * F), 3 * F
                _run("k_gtsa_attn", 0.0, lib.se_gtsa_attn, _p(qkv), kn, vn, _p(kc), _p(vc), _p(att), _p(a.delta), ldk, ldk, Fs, S, B, U, Hh, D, T, maxlen, F, st())
                tape(kn, vn, kc, vc, ko, vo, ldk, U, Hh, D)
                del qkv
                o = K._gemm(att, w["wo"], a.linear.bias)                  # [rows][F]
                _run("k_gtsa_addnorm", 0.0, lib.se_gtsa_addnorm, _p(o), F, _p(x), _p(x), _p(layer.norm_a.weight), _p(layer.norm_a.bias), S * 5, T, F, Fs, st())
                hid = K._gemm(x.view(rows, Fs), w["win"], layer.linear_in.bias, act=1)
                o = K._gemm(hid, layer.linear_out.weight, layer.linear_out.bias)
                del hid
                _run("k_gtsa_addnorm", 0.0, lib.se_gtsa_addnorm, _p(o), F, _p(x), _p(x), _p(layer.norm_i.weight), _p(layer.norm_i.bias), S * 5, T, F, Fs, st())
                del o
            else:
                qkv = _new(S, F, T, 16, dev=dev)
                _run("k_gtsa_qkv5", 0.0, lib.se_gtsa_qkv5, _p(x), _p(a.ql.weight), _p(a.ql.bias), _p(a.kl.weight), _p(a.kl.bias), _p(a.vl.weight),
                     _p(a.vl.bias), _p(qkv), S, T, F, Fs, st())
                kn, vn = _p(qkv, 5), _p(qkv, 10)
                at5 = _new(S, F, T, 8, dev=dev)
                _run("k_gtsa_attn", 0.0, lib.se_gtsa_attn, _p(qkv), kn, vn, _p(kc), _p(vc), _p(at5), _p(a.delta), 16, 16, 8, S, B, U, Hh, D, T, maxlen, 5, st())
                tape(kn, vn, kc, vc, ko, vo, 16, U, Hh, D)
                del qkv
                _run("k_gtsa_tail5", 0.0, lib.se_gtsa_tail5, _p(at5), 8, _p(x), _p(x), _p(a.linear.weight), _p(a.linear.bias), _p(layer.norm_a.weight),
                     _p(layer.norm_a.bias), _p(layer.linear_in.weight), _p(layer.linear_in.bias), _p(layer.linear_out.weight), _p(layer.linear_out.bias),
                     _p(layer.norm_i.weight), _p(layer.norm_i.bias), S, T, F, Fs, fn, st())
                del at5
            state["k"][i], state["v"][i] = ko, vo
        A = _new(S * T, 15 * Fs, dev=dev)
        _run("k_gtsa_gather3", 0.0, lib.se_gtsa_gather3, _p(x), _p(state["buf"]), _p(A), S, B, T, Fs, st())
        if cnt is None:
            state["buf"] = x[S - B:, :, T - 2:, :].contiguous()
        else:
            buf = torch.empty_like(state["buf"])
            _run("k_gtsa_lastframes", 0.0, lib.se_gtsa_lastframes_rows, _p(x), _p(state["buf"]), _p(buf), _ip(cnt), Nc, B, T, Fs, st())
            state["buf"] = buf
        g1 = K._gemm(A, conv_w["w1"], conv_w["b1"])
        del A
        g2 = K._gemm(g1, conv_w["w2"], conv_w["b2"])                     # [S T][2 * 2F]: conv_trans | conv_gated
        lc = self.last_conv
        Y = _new(S, T, F, 2, dev=dev)
        _run("k_gtsa_out", 0.0, lib.se_gtsa_out, _p(g2), 4 * F, _p(lc.norm.weight), _p(lc.norm.bias), _p(spec), _p(Y), None, S, M, T, F, st())
        istft_into(plan, sig, Y, ysegs[0], n0, Nc)

    @torch.no_grad()
    def _kernel_process(self, mixture, plan):
        """One call on the kernels, uniform or chains: StreamingMixin._prefix_passes' schedule over `_kernel_pass`."""
        dev, maxlen, Fs = mixture.device, self._cfg["maxlen"], (self.num_freqs + 7) // 8 * 8
        old = self._kstate if plan.any_flag else None

        def fresh(B):
            shapes = [self._seq_shape(i) for i in range(len(self.layers))]
            return dict(k=[torch.zeros(B * U * Hh, maxlen, D, device=dev) for U, Hh, D in shapes],
                        v=[torch.zeros(B * U * Hh, maxlen, D, device=dev) for U, Hh, D in shapes], buf=torch.zeros(B, 5, 2, Fs, device=dev))
        carried = None if old is None else {k: old[k] for k in ("k", "v", "buf")}
        (pred,), new, passes = self._prefix_passes(mixture, plan, carried, fresh, 1, self._kernel_pass)
        self._kstate = dict(B=mixture.shape[0], **new)
        self._last_passes = passes
        return pred
