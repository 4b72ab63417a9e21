"""Drop-in `TemporalCRN` for the reference's model-class contract.

Same constructor kwargs as reference CRN.py:415-417 (so `TemporalCRN(**config['TemporalCRN'])` with the
reference's config.yaml works unchanged), same `state_dict()` keys and shapes (incl. the `net.0.*` aliases,
CRN.py:314-316; ConvTranspose weights are [Cin, Cout, 5, 3]), same entry points:

    realtime_process(mixture[B, M, L], flag=False) -> [B, L]     CRN.py:560-589
    forward(x[B, M, F, T, 2]) -> [B, F, T, 2]                     CRN.py:454-496   (stateful)
    reset()                                                        CRN.py:498-503
    compute_loss(source, pred_source, length) -> (loss, stoi, sisnr)   CRN.py:593-617

The torch sub-modules below exist ONLY to own the parameters under the reference's names; no arithmetic runs
through them.  All compute goes through the C ABI (include/se_engine.h -> libse_engine.so, HIP on MI355X).
There is no CPU path: with CPU tensors or without the extension the calls raise.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import engine as _engine


class _Norm(nn.Module):  # GlobalLayerNorm parameter holder, CRN.py:120-132
    def __init__(self, dim, last=False):
        super().__init__()
        shape = (1, 1, 1, dim) if last else (1, dim, 1, 1)
        self.weight = nn.Parameter(torch.ones(shape))
        self.bias = nn.Parameter(torch.zeros(shape))


class _Conv(nn.Module):  # TemporalConv2d parameter holder, CRN.py:300-319; CRN_ELU.py:222-230 adds the gated 1x1 pair
    def __init__(self, cin, cout, kernel, stride, dil, dropout, gated=False):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel, stride=stride, padding=(2 * dil[0], 0), dilation=dil)
        if gated:  # registration order matters: it is the reference's state_dict order
            self.conv_trans = nn.Conv2d(cout, cout, 1, stride=1, padding=0)
            self.conv_gated = nn.Conv2d(cout, cout, 1, stride=1, padding=0)
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)
        self.norm = _Norm(cout)


class _Deconv(nn.Module):  # TemporalConvTranspose2d parameter holder, CRN.py:355-377
    def __init__(self, cin, cout, ks, dil, dropout):
        super().__init__()
        self.conv = nn.ConvTranspose2d(cin, cout, (5, ks), stride=(2, 1), padding=(2, 0), dilation=(1, dil))
        self.dropout = nn.Dropout(dropout)
        self.net = nn.Sequential(self.conv, self.dropout)
        self.residualmask = nn.Conv2d(cout, cout, (1, 1))
        self.residualnorm = _Norm(cout)
        self.residual = nn.Conv2d(cout, cout, (1, 1))
        self.norm = _Norm(cout)


class _Seq(nn.Module):  # SequenceModel parameter holder, CRN.py:196-254
    def __init__(self, size, hidden, num_layers):
        super().__init__()
        self.sequence_model = nn.GRU(input_size=size, hidden_size=hidden, num_layers=num_layers, batch_first=True)
        self.fc_output_layer = nn.Linear(hidden, size)
        self.norm = _Norm(size, last=True)


class TemporalCRN(nn.Module):
    _VARIANT = 0  # 0 = CRN.py; subclasses: 1 = CRN_ELU.py (crn_elu.TemporalCRN), 2 = distillation_crn.py student

    def __init__(self, num_channels, num_freqs, hidden, segment_length, num_layers=1, num_inputs=3, kernel_size=3,
                 dropout=0.0, sample_rate=16000, win_length=25, hop_length=10, n_fft=400):
        super().__init__()
        if dropout != 0.0:
            raise NotImplementedError("dropout > 0 is a training-only knob; the reference configs use 0.0 (config.yaml:213)")
        self.segment_length = segment_length
        self.num_freqs = num_freqs
        self._cfg_args = dict(num_channels=list(num_channels), num_freqs=num_freqs, hidden=hidden, segment_length=segment_length,
                              num_layers=num_layers, num_inputs=num_inputs, kernel_size=kernel_size, sample_rate=sample_rate,
                              win_length=win_length, hop_length=hop_length, n_fft=n_fft, variant=self._VARIANT)
        L = len(num_channels)
        gated = self._VARIANT != 0
        if gated:  # CRN_ELU.py:335-340: three 5x5 blocks with frequency dilation 1, 2, 4
            c0 = 2 * num_inputs - 1
            self.preconvlist = nn.ModuleList([_Conv(c0, c0, (5, 5), (1, 1), (fd, 1), dropout, gated=True) for fd in (1, 2, 4)])
        convs, deconvs = [], []
        for i in range(L):  # CRN.py:431-444
            cin = (2 * num_inputs - 1) if i == 0 else num_channels[i - 1]
            cout = num_channels[i]
            convs.append(_Conv(cin, cout, (5, kernel_size), (2, 1), (1, 2 ** i), dropout, gated=gated))
            d = 2 ** (L - i - 1)
            deconvs.insert(0, _Deconv(cout, 2 if i == 0 else cin, kernel_size, d, dropout))
        self.convlist = nn.ModuleList(convs)
        self.deconvlist = nn.ModuleList(deconvs)
        size = (num_freqs // 16 + 1) * num_channels[-1]
        self.gru = _Seq(size, hidden, num_layers)
        self._eng: Optional[_engine.Engine] = None
        self._eng_device = None
        self._eng_precision = 0
        self._precision_request = None  # set_precision(): None = follow the parameter dtype (fp32 -> 0, fp16 -> 1)
        self._versions = None

    # ---- engine plumbing -------------------------------------------------------------------------------
    def _engine_for(self, t: torch.Tensor) -> _engine.Engine:
        if not t.is_cuda:
            raise RuntimeError("TemporalCRN runs on the MI355X engine only: move the model and inputs to the GPU "
                               "(there is no CPU fallback; the CPU restatement lives in oracle/ for tests)")
        dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        # model.half() (the fp16 inference idiom) selects fp16 MFMA operands; set_precision("bf16x3") the 3-term split-bf16
        # mode that stays inside the 1e-4 parity bar (BASELINE config 5's fast mode)
        precision = self._precision_request
        if precision is None:
            precision = 1 if next(self.parameters()).dtype == torch.float16 else 0
        if self._eng is None or self._eng_device != dev or self._eng_precision != precision:
            self._eng = _engine.Engine(_engine.make_config(**self._cfg_args, precision=precision), dev)
            self._eng_device = dev
            self._eng_precision = precision
            self._versions = None
        versions = tuple(p._version for p in self.parameters())
        if versions != self._versions:  # weights changed (load_state_dict, optimizer step, ...): re-upload
            self._eng.load_state_dict({k: v for k, v in self.state_dict().items()})
            self._versions = versions
        return self._eng

    _PRECISIONS = {"fp32": 0, "f32": 0, "fp16": 1, "f16": 1, "bf16x3": 2}

    def set_precision(self, mode):
        """Extension over the reference: contraction arithmetic of the engine.  "fp32" (default) = fp32-accurate 6-term
        split-bf16 MFMA; "bf16x3" = 3-term split-bf16 (16 mantissa bits per operand, fp32 accumulate), inside the 1e-4 RMS /
        0.02 dB parity bar at half the matrix work; "fp16" = fp16 operands (outside the bar, ~2e-3); None = follow the dtype."""
        if mode is not None and mode not in self._PRECISIONS:
            raise ValueError(f"precision {mode!r} not in {sorted(self._PRECISIONS)}")
        self._precision_request = None if mode is None else self._PRECISIONS[mode]
        return self

    # ---- reference contract --------------------------------------------------------------------------
    def reset(self):
        if self._eng is not None and self._eng.batch > 0:
            self._eng.reset(self._eng.batch)

    def reset_stream(self, index: int):
        """Extension over the reference (which can only reset the whole batch): reset one stream's conv buffers and GRU
        state so that a new caller can take that batch slot while the other streams keep their state."""
        if self._eng is None or self._eng.batch <= 0:
            raise RuntimeError("reset_stream before any state exists")
        self._eng.reset_stream(index)

    def forward(self, x):
        eng = self._engine_for(x)
        if eng.batch != x.shape[0]:
            eng.reset(x.shape[0])  # lazy state allocation on first call, CRN.py:325-326
        return eng.forward(x.contiguous().float())

    def realtime_process(self, mixture, flag=False, lengths=None):
        """lengths: extension over the reference - a ragged batch (zero-padded to the longest utterance): every stream is processed as if
        alone with its own length (own padding; zeros beyond its length in the output).
        flag: a bool or a one-element tensor (the reference trainer's flag) for the whole batch; a sequence or tensor with one value per
        stream makes the call a batch of chunk chains (Engine.realtime_process_chains): stream b continues its own state where flag[b] is
        set, starts afresh where it is not, and every stream leaves the state it would carry alone."""
        eng = self._engine_for(mixture)
        return eng.realtime_process(mixture.contiguous().float(), flag=flag, lengths=lengths)

    def compute_loss(self, source, pred_source, length):
        """loss = 0.7 * stoi_loss + 0.3 * (-SI-SNR), NaN -> zeros  (CRN.py:593-617); returns (loss, stoi, sisnr) on the
        device of `pred_source` with gradients to it.  See losses.py: device-resident restatement of utility.stoi_loss
        (torchaudio boundary unpinned) and a fused HIP SI-SNR kernel pair."""
        from .losses import compute_loss
        return compute_loss(source, pred_source, length)
