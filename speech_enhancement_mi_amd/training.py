"""Data-parallel training path (BASELINE config 4): utterances sharded across the GPUs of one node,
ONE flat fp32 gradient bucket all-reduced per optimizer step over RCCL/xGMI.

`TrainableCRN` has two interchangeable differentiable forwards of `realtime_process` (CRN.py:560-589):
  * `use_hip_kernels(True)`: every stage forward AND backward on the hand-written kernels (train_net.CRNFunction;
    SURVEY.md 8f-1) - the path bench.py --mode train times;
  * default: a PyTorch autograd restatement of the same arithmetic, CPU-runnable, pinned against the CPU oracle
    (tests/test_training_cpu.py) - the checker the GPU tests compare the kernels with.
Around it: the flat-bucket gradient all-reduce the reference never had (its DDP lines are commented out,
train.py:172-173,252-256) and the optimizer step of the reference trainer (Adam 3e-4, grad-accum 2, clip 5;
train.py:198-204, config.yaml:9,99).  Loss: `compute_loss` = 0.7 * stoi_loss + 0.3 * (-SI-SNR) (CRN.py:609-611; losses.py:
HIP SI-SNR kernels + the batched device-resident STOI restatement, torchaudio boundary unpinned) or the SI-SNR term alone.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as Fn

from .crn import TemporalCRN
from .crn_elu import TemporalCRN as TemporalCRNELU
from .distillation_crn import TemporalCRN as TemporalStudentCRN
from .losses import cal_si_snr
from .call_plan import as_flags, as_lengths, call_plan, istft_windows, overlap_add_cut, segment_geometry, stft_windows, windows

EPS = 1e-8


def _gln(x, w, b, eps_mode=0):
    """GlobalLayerNorm(time=False), CRN.py:135-149: per-sample stats over all non-batch dims.  eps_mode 1: the denominator
    sqrt(var) + EPS of distillation_crn.py:51 (variant 2)."""
    dims = tuple(range(1, x.dim()))
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    sd = torch.sqrt(var) if eps_mode else torch.sqrt(var + EPS)
    return (x - mean) / (sd + EPS) * w + b


class _TrainableMixin:
    """Differentiable `realtime_process` on top of the drop-in parameter holders (crn.TemporalCRN / crn_elu.TemporalCRN).  Same
    parameters / state_dict as the inference shim, so a checkpoint trained here loads into the HIP engine unchanged."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        c = self._cfg_args
        self._win = int(round(c["sample_rate"] / 1000.0 * c["win_length"]))
        self._hop = int(round(c["sample_rate"] / 1000.0 * c["hop_length"]))
        self._nfft = c["n_fft"]
        self._state = None
        self._hip = False
        self._hip_state_from_torch = False

    def use_hip_kernels(self, flag=True):
        """True: the whole differentiable realtime_process - STFT, features, convolutions, norms, GRU, dense layers, skip gates,
        mask, iSTFT, overlap-add - runs forward AND backward on the hand-written kernels (train_net.CRNFunction: one autograd
        node, no float atomics); False (default): torch ops + autograd, the CPU-runnable checker the tests pin to the oracle."""
        if bool(flag) != self._hip:
            self._state = None  # the two paths keep their carried state in different layouts
        self._hip = bool(flag)
        self._hip_state_from_torch = False
        return self

    # ---- signal glue (utility.py:312-403, CRN.py:505-520) ----
    def _segment(self, x):
        """utility.segmentation of x [B, M, L] as it stands (no lead): call_plan.windows of a continuing call -> ([B, M, N, K], gap)"""
        plan = call_plan(True, None, x.shape[0], x.shape[-1], self.segment_length, self.segment_length, 0)   # the STFT sizes do not enter
        return windows(plan, x), plan.gap

    def _stft(self, seg):  # [..., K] -> [..., F, T] complex
        return stft_windows(seg, self._nfft, self._hop, self._win, torch.float32)

    def _istft(self, spec):  # [..., F, T] complex -> [..., K]
        return istft_windows(spec, self._nfft, self._hop, self._win, torch.float32)

    # ---- one segment, CRN.py:454-496 (variant 0) / CRN_ELU.py:367-407 (variant 1) / distillation_crn.py:337-380 (variant 2) ----
    def _forward_segment(self, X, state, feats=None):
        """X [B, M, F, T] complex; state = dict(buf=[...], h=tensor|None, pbuf=[...]) (detached, like CRN.py:281,334).
        feats: a list that receives the five distillation feature maps [B, C, F, T] (distillation_crn.py:451-477)."""
        V = self._VARIANT
        em = 1 if V == 2 else 0  # gLN denominator sqrt(var) + EPS (distillation_crn.py:51)
        actf = Fn.elu if V else torch.relu
        re, im = X.real, X.imag
        ang = torch.atan2(im, re) if V == 1 else torch.atan(im / (re + EPS) + EPS)
        mag = torch.sqrt(re ** 2 + im ** 2 + 1e-10)
        x = torch.cat([mag, ang[:, :1] - ang[:, 1:]], dim=1)

        def gated(blk, a):  # CRN_ELU.py:240
            return Fn.conv2d(a, blk.conv_trans.weight, blk.conv_trans.bias) * torch.sigmoid(Fn.conv2d(a, blk.conv_gated.weight, blk.conv_gated.bias))

        new_pbuf = []
        if V:
            for k, blk in enumerate(self.preconvlist):  # x = block(x) + x, CRN_ELU.py:375-376
                fd = 2 ** k
                buf = state["pbuf"][k] if state.get("pbuf") is not None else x.new_zeros(x.shape[0], x.shape[1], x.shape[2], 4)
                y = Fn.conv2d(torch.cat([buf, x], dim=-1), blk.conv.weight, blk.conv.bias, stride=(1, 1), padding=(2 * fd, 0), dilation=(fd, 1))
                new_pbuf.append(x[..., -4:].detach())
                x = _gln(gated(blk, actf(y)), blk.norm.weight, blk.norm.bias, em) + x
        residuals = [x]
        new_buf = []
        for i, blk in enumerate(self.convlist):
            d = 2 ** i
            P = 2 * d
            buf = state["buf"][i] if state["buf"] is not None else x.new_zeros(x.shape[0], x.shape[1], x.shape[2], P)
            inp = torch.cat([buf, x], dim=-1)
            y = Fn.conv2d(inp, blk.conv.weight, blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=(1, d))
            new_buf.append(x[..., -P:].detach())
            x = _gln(gated(blk, actf(y)) if V else actf(y), blk.norm.weight, blk.norm.bias, em)
            residuals.append(x)
        if feats is not None:
            feats.append(y)  # ft0: the last encoder convolution before ELU
        B, C, Fq, T = x.shape
        seq = x.reshape(B, C * Fq, T).permute(0, 2, 1)
        o, h = self.gru.sequence_model(seq, state["h"])
        o = self.gru.fc_output_layer(o)
        if feats is not None:
            feats.append(o.reshape(B, C, Fq, T))  # ft1: [B, T, D] reshaped, not permuted (distillation_crn.py:368)
        o = actf(o)
        o = _gln(o.unsqueeze(1), self.gru.norm.weight, self.gru.norm.bias, em).squeeze(1)
        x = o.permute(0, 2, 1).reshape(B, C, Fq, T)
        L = len(self.deconvlist)
        for j, blk in enumerate(self.deconvlist):
            d = 2 ** j
            y = Fn.conv_transpose2d(x, blk.conv.weight, blk.conv.bias, stride=(2, 1), padding=(2, 0), dilation=(1, d))[..., -T:]
            if feats is not None and j < L - 1:
                feats.append(y)  # ft2..: the transposed-convolution outputs before activation
            y = _gln(actf(y), blk.norm.weight, blk.norm.bias, em)
            if j < L - 1:
                res = residuals[-2 - j]
                if res.shape[2] > y.shape[2]:
                    y = Fn.pad(y, (0, 0, 0, res.shape[2] - y.shape[2]))
                elif res.shape[2] < y.shape[2]:
                    y = y[:, :, :res.shape[2]]
                m = torch.sigmoid(_gln(Fn.conv2d(res, blk.residualmask.weight, blk.residualmask.bias), blk.residualnorm.weight, blk.residualnorm.bias, em))
                y = m * actf(Fn.conv2d(res, blk.residual.weight, blk.residual.bias)) + (1.0 - m) * y
            x = y
        m = x.clamp(-9.9, 9.9)  # decompress_cIRM, utility.py:439-442 (the clamp has zero gradient outside, like the reference's masks)
        m = -10.0 * torch.log((10.0 - m) / (10.0 + m))
        Y = torch.complex(m[:, 0] * re[:, 0] - m[:, 1] * im[:, 0], m[:, 1] * re[:, 0] + m[:, 0] * im[:, 0])
        return Y, dict(buf=new_buf, h=h.detach(), pbuf=new_pbuf if V else None)

    def _zero_state(self, B, M, like):
        """The state of B utterances after a reset, spelled out (what `None` stands for in _forward_segment)"""
        g = self.gru.sequence_model
        ch = [2 * M - 1] + [blk.conv.weight.shape[0] for blk in self.convlist]
        Fq = segment_geometry(1, True, self.segment_length, self._hop, self._nfft, ch)["Fq"]
        return dict(buf=[like.new_zeros(B, ch[i], Fq[i], 2 * 2 ** i) for i in range(len(self.convlist))], h=like.new_zeros(g.num_layers, B, g.hidden_size),
                    pbuf=[like.new_zeros(B, ch[0], Fq[0], 4) for _ in self.preconvlist] if self._VARIANT else None)

    @staticmethod
    def _merge_state(mask, a, b):
        """per utterance: a where mask [B] holds, else b"""
        pick = lambda x, y, bdim: torch.where(mask.view([-1 if d == bdim else 1 for d in range(x.dim())]), x, y)
        return dict(buf=[pick(x, y, 0) for x, y in zip(a["buf"], b["buf"])], h=pick(a["h"], b["h"], 1),
                    pbuf=None if a["pbuf"] is None else [pick(x, y, 0) for x, y in zip(a["pbuf"], b["pbuf"])])

    def realtime_process_train(self, mixture, flag=False, features=False, lengths=None):
        """Differentiable realtime_process (CRN.py:560-589): [B, M, L] -> [B, L].  features=True (variant 2): returns (pred, [ft0..ft4])
        with the five distillation feature maps [N*B, C, F, T], window-major (distillation_crn.py:451-477).
        flag as one value per utterance ([B] tensor / list) and / or lengths ([B] ints <= L): the batch is B independent chunk chains
        (train_net.realtime_process_fused states the contract; both paths honour it).  Here: every statistic of the model is per utterance
        and segment positions do not depend on the length, so all utterances run the N = max N_b segments of the longest; an utterance's
        carried state is taken after its OWN last segment, its output cut from its own samples.  The uniform call is that loop with one
        flag and N_b = N for all (bit for bit what a loop without the per-utterance merges gives)."""
        if features and self._VARIANT != 2:
            raise ValueError("feature maps exist for the distillation_crn.py architecture (variant 2) only")
        if self._hip:  # every stage forward and backward on the hand-written kernels, one autograd node (train_net.py)
            from .train_net import realtime_process_fused
            if self._hip_state_from_torch:
                raise RuntimeError("flag=True continuation across a use_hip_kernels() switch is not supported: start with flag=False")
            return realtime_process_fused(self, mixture, flag, features=features, lengths=lengths)
        B, M, Lmax = mixture.shape
        plan = call_plan(flag, lengths, B, Lmax, self.segment_length, self._hop, self._nfft)
        dev = mixture.device
        if plan.uniform:   # one flag: the carried state as it stands, or None entries = zeros (_forward_segment)
            state = self._state if plan.flag else dict(buf=None, h=None, pbuf=None)
        else:
            state = self._zero_state(B, M, mixture)
            if plan.any_flag:
                if self._state is None or self._state.get("buf") is None or self._state["h"].shape[1] != B:
                    raise RuntimeError(f"flag=True continues row b of the carried state of {B} utterances: there is none")
                state = self._merge_state(torch.tensor(plan.flags, device=dev), self._state, state)
        X = self._stft(windows(plan, mixture))  # [B, M, N, F, T]
        Nb = torch.tensor(plan.Nb, device=dev)
        final, outs, fts = state, [], []
        for n in range(plan.N):
            f = [] if features else None
            Y, state = self._forward_segment(X[:, :, n], state, f)
            outs.append(self._istft(Y))
            fts.append(f)
            if not plan.uniform and n + 1 in plan.Nb:
                final = self._merge_state(Nb == n + 1, state, final)
        self._state = state if plan.uniform else final
        out = overlap_add_cut(plan, torch.stack(outs, dim=1))  # [B, N, K] -> [B, L]
        if features:
            return out, [torch.cat([f[k] for f in fts], dim=0) for k in range(len(fts[0]))]
        return out


class TrainableCRN(_TrainableMixin, TemporalCRN):
    """CRN.py TemporalCRN (variant 0), trainable."""


class TrainableCRNELU(_TrainableMixin, TemporalCRNELU):
    """CRN_ELU.py TemporalCRN (variant 1) - the model the reference's train.py imports and trains (train.py:16)."""


class TrainableStudentCRN(_TrainableMixin, TemporalStudentCRN):
    """distillation_crn.py TemporalCRN (variant 2: arctan phase, gLN denominator sqrt(var) + EPS), the teacher and the student of
    distillation_crn.DistillationCRN.  realtime_process stays the inference engine (weights re-uploaded after every optimizer step);
    realtime_process_train(..., features=True) is the differentiable forward with the five feature maps."""


def si_snr_loss(pred, source, length=None):
    """The SI-SNR term of compute_loss (CRN.py:610): -cal_si_snr(pred, source, length)."""
    return -cal_si_snr(pred, source, length)


class FlatBucket:
    """One contiguous fp32 gradient buffer for all parameters (24.46 MB for the CRN); every p.grad is a view
    into it, so backward accumulates in place and the data-parallel exchange is ONE all-reduce per optimizer step."""

    def __init__(self, params: List[torch.nn.Parameter]):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def zero(self):
        self.flat.zero_()

    def all_reduce_mean(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)  # RCCL over xGMI with backend "nccl"
            self.flat.div_(dist.get_world_size())

    def clip_(self, max_norm: float) -> float:
        """clip_grad_norm_ on the REDUCED gradients, so every rank clips identically (train.py:200)."""
        norm = float(self.flat.norm())
        if norm > max_norm:
            self.flat.mul_(max_norm / (norm + 1e-6))
        return norm


def train_step(model: TrainableCRN, bucket: FlatBucket, optimizer, mixture, source, length=None, accum: int = 1, loss: str = "sisnr", merge=None,
               flag=None):
    """One optimizer step of the reference trainer (train.py:195-204) under data parallelism: `accum` micro-batches of local
    utterances, one flat all-reduce, clip 5, Adam.  loss = "full": 0.7 * stoi_loss + 0.3 * (-SI-SNR) (compute_loss,
    CRN.py:609-611); "sisnr": the SI-SNR term alone.

    merge (default: on for the hand-written kernels): gradient accumulation exists to bound memory; every statistic of the model
    is per utterance, so the `accum` micro-batches can share ONE forward / backward sweep (half the dependent GRU steps) while
    the loss is still formed per micro-batch, sum_i loss(micro-batch i) / accum - the same function of the parameters, hence
    the same gradient up to fp32 summation order (tests/test_gpu_round3.py::test_merged_microbatches_give_the_accumulated_gradient).
    merge=False runs the micro-batches one after the other like the reference loop.

    flag (a bool, or one value per utterance; default None = every call starts afresh and the forward sees the whole padded batch, as
    before): the batch is one step of B chunk chains (datagen.ChunkChainBatch); flag and `length` reach the forward as its per-utterance
    flags and lengths, and the model keeps every utterance's own state for the next step."""
    bucket.zero()
    total = 0.0
    if merge is None:
        merge = model._hip
    srcs = source.chunk(accum)
    lens = [None] * len(srcs) if length is None else list(length.chunk(accum))

    def loss_of(pred, src, ln, slot=0):
        if loss == "full":
            ll = ln if ln is not None else torch.full((pred.shape[0],), pred.shape[-1], dtype=torch.int64, device=pred.device)
            return model.compute_loss(src, pred, ll)[0] / accum
        return si_snr_loss(pred, src, ln) / accum

    B = mixture.shape[0]
    chain = [{}] * accum   # the forward's flag / lengths per micro-batch
    if flag is not None:
        flags, lns = as_flags(flag, B), as_lengths(length, B, mixture.shape[-1])
        per = -(-B // accum)   # torch.chunk's split
        chain = [dict(flag=flags[i:i + per], lengths=lns[i:i + per]) for i in range(0, B, per)]
    if merge:
        pred = model.realtime_process_train(mixture, **(dict(flag=flags, lengths=lns) if flag is not None else {}))
        val = None
        for slot, (p_i, src, ln) in enumerate(zip(pred.chunk(accum), srcs, lens)):
            v = loss_of(p_i, src, ln, slot)
            val = v if val is None else val + v
        val.backward()
        total = float(val.detach())
    else:
        if flag is not None and any(flags) and accum > 1:
            raise ValueError("one model carries one batch of states: chunk chains with flag=True need merge=True (or accum=1)")
        for mix, src, ln, kw in zip(mixture.chunk(accum), srcs, lens, chain):
            val = loss_of(model.realtime_process_train(mix, **kw), src, ln)
            val.backward()
            total += float(val.detach())
    if model._hip:
        from . import train_ops
        train_ops.pseq_check()  # a persistent GRU launch that gave up its bounded spin must not go unnoticed
    bucket.all_reduce_mean()
    bucket.clip_(5.0)
    optimizer.step()
    return total
