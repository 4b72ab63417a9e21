"""What the Python drop-ins that stream through `realtime_process` share (general_beamformer.GeneralBeamformer, gtsa.GTSA): the call's
contract, the choice of path, the refusals, the carried state, the torch restatement's signal chain, the kernel path's prologue and the
kernel path's schedule for chunk chains (`_prefix_passes`).

    realtime_process(mixture [B, M, L], flag=False, lengths=None) -> [B, L]

flag: a bool, ONE value, or one per utterance ([B] tensor / list); lengths: per-utterance lengths <= L (None: all full).  With either
given per utterance the batch is B independent CHUNK CHAINS (call_plan.py, datagen.ChunkChainBatch): utterance b is
mixture[b, :, :lengths[b]] (whatever the padding holds), starts from zero state where flag[b] is False and continues row b of the
carried state where it is True; pred[b, lengths[b]:] = 0, and the carried state afterwards holds, per utterance, what that utterance
alone would carry.  A batch whose flags and lengths are all alike is a UNIFORM call, as a bool flag is; a uniform flag=True call with
nothing carried starts from zeros, as the reference does.

The state lives per path: `_tstate` (torch restatement) and `_kstate` (kernels), `_last_path` = "torch" / "kernel" says whose turn the
last call was.  Refused, in this order and before any state is read or written:
  * a flag set while the carried state belongs to the other path                               RuntimeError ("other path")
  * chains with a flag set and no carried state, or one of another batch size                  ValueError ("there is none" / "one of N")
  * a uniform flag=True call whose batch size differs from the carried one                     ValueError naming both sizes
and a call that is refused or fails leaves the carried state it found: both paths build the new state out of place and store it when
the call has succeeded (the one exception: a persistent-GRU time-out clears `_kstate`, the output being invalid).

hifigan.Generator shares the mixin too: its `realtime_process(mixture, post, reset)` and `realtime_process_chains(mixture, resets,
lengths, post)` have two results and `reset` = not `flag`, so it parses its own arguments and takes the choice of path and the refusals
from `_admit`; its chains on the restatement run every stream alone as `_torch_call` does, with the norm state that no reset clears.

The kernel path's chains (GTSA, hifigan.Generator; GeneralBeamformer runs every stream in every pass): `_prefix_passes` sorts the streams
by window count, so the streams still running at window n0 are a prefix, and hands the model's pass that prefix only.  It knows the state
as a dict from name to a tensor or a list of tensors, every one stream-major with a multiple of B rows, and nothing else of the model.

A model provides `segment_length`, `_cfg["n_fft"]` and
    _choose_path(mixture) -> "torch", "kernel" or the name X of a path of its own on the kernel state (`_X_call(mixture, plan)`);
                             default: the kernels for a GPU tensor in eval mode with grad disabled
    _plan_channels(M)                  the U-Net levels' channels for the plan's geometry (default: none)
    _batch_of(state) -> B              of either state
    _torch_windows(X [B, M, N, F, T, 2], state | None) -> (Y [B, N, F, T, 2], state)     the restatement's windows, out of place
    _state_row(state, b, B), _state_merge([one-row states])                               the restatement's chains: every utterance alone
    kernel_geometry_error() -> None | str,  _kernel_process(mixture contiguous fp32, plan) -> pred; stores `_kstate` at its end
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from . import train_ops as K
from .call_plan import CallPlan, call_plan, chain_passes, istft_windows, overlap_add_cut, stft_windows, windows
from .train_stages import _new, _rows, _sig, overlap_add, slab_gather

_DEFAULT_MAX_SEGMENTS = 8


def _each(fn, state, *more):
    """{name: fn(name, t, the same tensor of every further state)} over the tensors t of a state, its lists kept as lists"""
    return {k: [fn(k, *ts) for ts in zip(v, *(m[k] for m in more))] if isinstance(v, list) else fn(k, v, *(m[k] for m in more))
            for k, v in state.items()}


class StreamingMixin:
    def _init_streaming(self, mics, sample_rate, win_length, hop_length):
        self._mics = mics
        self._win = int(round(sample_rate / 1000.0 * win_length))
        self._hop = int(round(sample_rate / 1000.0 * hop_length))
        self.max_segments = _DEFAULT_MAX_SEGMENTS   # windows per kernel pass (GTSA: per restatement tape pass too): bounds peak memory
        self._hip = True
        self._tstate = None
        self._kstate = None
        self._last_path = None
        self._derived = {}
        self.taps = None      # restatement forward(): set to {} to receive its intermediate tensors

    def reset(self):
        self._tstate = None
        self._kstate = None

    def use_hip_kernels(self, flag=True):
        """True (default): realtime_process runs on the kernels where the model's _choose_path allows; False: always the restatement."""
        self._hip = bool(flag)
        return self

    def _plan_channels(self, M):
        return ()

    def _choose_path(self, mixture):
        return "kernel" if self._hip and mixture.is_cuda and not torch.is_grad_enabled() and not self.training else "torch"

    def _plan(self, flag, lengths, B, L, M):
        return call_plan(flag, lengths, B, L, self.segment_length, self._hop, self._cfg["n_fft"], self._plan_channels(M))

    def realtime_process(self, mixture, flag=False, lengths=None):
        """The contract, the refusals and the rule for the carried state: this module's docstring."""
        B, M, L = mixture.shape
        plan = self._plan(flag, lengths, B, L, M)
        return getattr(self, f"_{self._admit(mixture, plan)}_call")(mixture, plan)

    def _admit(self, mixture, plan):
        """The choice of path and the refusals of a call -> the name of the path that runs it (a model whose realtime_process has
        another signature, hifigan.Generator, parses its own arguments into a plan and comes here)."""
        B = mixture.shape[0]
        run = self._choose_path(mixture)
        path = "torch" if run == "torch" else "kernel"
        if plan.any_flag:
            state = self._tstate if path == "torch" else self._kstate
            have = None if state is None else self._batch_of(state)
            if self._last_path not in (None, path):
                raise RuntimeError("flag=True continues the state of the other path (kernels vs restatement): start with flag=False")
            if not plan.uniform and have != B:
                raise ValueError(f"flag=True continues row b of the carried state of a batch of {B} utterances: there is "
                                 f"{'none' if have is None else 'one of ' + str(have)}")
            if have not in (None, B):
                raise ValueError(f"flag=True continues a batch of {have} utterances, got {B}")
        self._last_path = path
        return run

    # ---- torch restatement ---------------------------------------------------------------------------------------------------
    def spectrum(self, seg):
        """stft_trans of the windows [B, M, N, K] -> [B, M, N, F, T, 2] (torch.stft; speechbrain's STFT wrapper)"""
        return torch.view_as_real(stft_windows(seg, self._cfg["n_fft"], self._hop, self._win, seg.dtype))

    def _restate(self, mixture, plan, state):
        """One uniform call on the restatement, out of place -> (pred [B, L], state)"""
        Y, state = self._torch_windows(self.spectrum(windows(plan, mixture)), state)
        y = istft_windows(torch.view_as_complex(Y.contiguous()), self._cfg["n_fft"], self._hop, self._win, mixture.dtype)
        return overlap_add_cut(plan, y), state

    def _torch_call(self, mixture, plan):
        """Uniform: the batch as it stands.  Chains (the oracle of the kernel paths): every utterance literally alone - B = 1, its own
        length and flag, its own row of the carried state - the outputs padded to the batch width, the states merged row by row."""
        B, M, Lmax = mixture.shape
        st = self._tstate
        if plan.uniform:
            pred, new = self._restate(mixture, plan, st if plan.flag else None)
        else:
            preds, rows = [], []
            for b, (f, L) in enumerate(zip(plan.flags, plan.lengths)):
                y, row = self._restate(mixture[b:b + 1, :, :L], self._plan(f, None, 1, L, M), self._state_row(st, b, B) if f else None)
                preds.append(Fn.pad(y, (0, Lmax - L)))
                rows.append(row)
            pred, new = torch.cat(preds), self._state_merge(rows)
        self._tstate = new
        return pred

    # ---- kernel path ---------------------------------------------------------------------------------------------------------
    def _kernel_call(self, mixture, plan):
        name = type(self).__name__
        err = self.kernel_geometry_error()
        if err:
            raise ValueError(f"{name} kernel path: {err}")
        K._need_gpu(mixture, next(self.parameters()))
        if mixture.shape[1] != self._mics:
            raise ValueError(f"{name} kernel path: {mixture.shape[1]} microphones, the model is built for {self._mics}")
        return self._kernel_process(mixture.contiguous().float(), plan)

    def _prefix_passes(self, mixture, plan, carried, fresh, nout, run_pass, unflagged=()):
        """The passes of one call on the kernels -> (nout predictions [B, L], the new state, the passes [(n0, Nc, Bp), ...]).
        carried: the state the call continues, {name: a tensor or a list of tensors}, every tensor stream-major with a multiple of B
        rows; None: nothing is carried, and fresh(B) makes the state a stream starts from.  run_pass(mix[:Bp], sub_plan, sig, state,
        n0, Nc, ysegs) runs windows [n0, n0 + Nc) of the sub-plan's streams - the leading Bp rows of mix and of every state tensor;
        the nout window buffers ysegs [N][B][Ks] may be wider - and advances `state` in place, out of place for every tensor.
        sub_plan.rows are the caller's rows of those streams.  unflagged: the entries that go on whatever the flag says.

        Chains: the streams are sorted by window count (descending, stable), so the streams with a window at n0 or later are a
        prefix: pass (n0, Nc, Bp) of call_plan.chain_passes runs on the leading Bp rows of the sorted mixture and working state.  The
        working state is gathered in that order - an unflagged entry as it stands, any other through ONE slab_gather whose table folds
        the sort and the flag together: the carried row where the flag is set, zeros elsewhere (start_rows' gather).  A stream leaves
        the working state for its row of the new state when the prefix drops it; the streams still in the prefix at the end follow.
        The predictions are un-sorted by the same index.  A uniform call is the identity order with all B streams in every pass:
        nothing is sorted, gathered or scattered, and the working state (from shallow copies of the carried lists) is the new one."""
        dev = mixture.device
        B, M, L = mixture.shape

        def part(rows):
            sub = CallPlan([plan.flags[b] for b in rows], [plan.lengths[b] for b in rows], L, self.segment_length, self._hop, self._cfg["n_fft"],
                           self._plan_channels(M), uniform=False)
            sub.rows = rows
            return sub

        if plan.uniform:
            sp, mix = plan, mixture
            state = fresh(B) if carried is None else {k: list(v) if isinstance(v, list) else v for k, v in carried.items()}
            ysegs = [_new(plan.N, B, plan.Ks, dev=dev) for _ in range(nout)]
        else:
            order = sorted(range(B), key=lambda b: -plan.Nb[b])
            order_dev = _rows(order, dev)
            sp, mix = part(order), mixture.index_select(0, order_dev)
            carry = None if carried is None else _rows([b if plan.flags[b] else -1 for b in order], dev)

            def start(name, t):
                if name in unflagged:
                    return t.view(B, -1).index_select(0, order_dev).view(t.shape)
                return t if carry is None else slab_gather(t, carry, B, t.numel() // B, t.numel() // B, 0).view(t.shape)
            state = _each(start, fresh(B) if carried is None else carried)
            new = _each(lambda _, t: torch.empty_like(t), state)
            ysegs = [torch.zeros(sp.N, B, sp.Ks, device=dev) for _ in range(nout)]   # windows a prefix pass never writes stay zero

        def retire(state, lo, cur):
            """rows [lo, cur) of the working state (cur streams, sorted) -> their own rows of the new state; rows [0, lo) stay"""
            def move(_, t, o):
                o.view(B, -1).index_copy_(0, order_dev[lo:cur], t.view(cur, -1)[lo:])
                return t[:t.shape[0] // cur * lo]
            return _each(move, state, new)

        sig = _sig(dev, self._cfg["n_fft"], self._win, self._hop, self.segment_length)
        passes = chain_passes(sp.Nb, self.max_segments)
        sub, cur = {B: sp}, B
        for n0, Nc, Bp in passes:
            if Bp < cur:   # chains only: a uniform plan keeps all B streams to the end
                state, cur = retire(state, Bp, cur), Bp
                sub[Bp] = part(order[:Bp])
            run_pass(mix[:Bp], sub[Bp], sig, state, n0, Nc, ysegs)
        preds = [overlap_add(sp, sig, y) for y in ysegs]
        if plan.uniform:
            return preds, state, passes
        retire(state, 0, cur)
        return [torch.empty(B, L, device=dev).index_copy_(0, order_dev, p) for p in preds], new, passes

    def _cached(self, name, params, make):
        """make() of some parameters (a derived weight: padded, stacked), once per parameter version"""
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._derived.get(name, (None,))[0] != key:
            with torch.no_grad():
                self._derived[name] = (key, make())
        return self._derived[name][1]
