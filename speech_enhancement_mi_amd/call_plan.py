"""What one `realtime_process` call looks like, decided once: the flag / lengths arguments parsed, and the segment geometry of the call.

Every training / kernel path accepts `flag` as a bool, ONE value (the reference trainer's flag tensor) or one value per utterance, and
optional per-utterance `lengths`.  `call_plan` reads them (a tensor once, here: nothing later synchronises), validates them and
triages: one flag for all and every utterance Lmax long is a UNIFORM call, carrying `segment_geometry`'s values and taking the scalar
kernels; anything else is a batch of B independent CHUNK CHAINS (datagen.ChunkChainBatch), carrying `ragged_geometry`'s and taking the
`_rows` kernels.  The result is a `CallPlan`; train_stages.py's signal-chain helpers, the three autograd Functions and the torch
restatements (`windows`, `stft_windows`, `istft_windows`, `overlap_add_cut` below) take it and never look at `flag` again.

Pure Python and torch-free at import (tensors are handled by duck typing), so engine.py and train_stages.py both import it: the
geometry arithmetic (`_chunk`) and the flag parser (`flags_of`) exist once.  tests/test_chain_plan_cpu.py holds the arithmetic equal
to the library's se_chunk_geometry.
"""
from __future__ import annotations


# ---- parsing ---------------------------------------------------------------------------------------------------------------------
def _is_tensor(v):
    return hasattr(v, "reshape") and hasattr(v, "tolist")


def flags_of(flag, B, error=RuntimeError, unit=""):
    """The flag argument of realtime_process: a bool or ONE value (the reference trainer's flag tensor) -> a bool; a sequence or tensor
    with one value per utterance -> a list of B bools (a mixed tensor stays mixed)."""
    if _is_tensor(flag):
        flag = flag.reshape(-1).tolist()
    if isinstance(flag, (list, tuple)):
        if len(flag) == 1:
            return bool(flag[0])
        if len(flag) != B:
            raise error(f"{len(flag)} flags for a batch of {B}{unit}")
        return [bool(f) for f in flag]
    return bool(flag)


def as_flag(flag):
    """One flag for the whole batch: a bool, or the trainer's flag tensor (data['flag'], shape [B]; one value per batch)"""
    return bool(flag.reshape(-1)[0].item()) if _is_tensor(flag) else bool(flag)


def as_flags(flag, B):
    """flags_of as a list of B bools whatever the form"""
    flags = flags_of(flag, B, ValueError, " utterances")
    return flags if isinstance(flags, list) else [flags] * B


def as_lengths(lengths, B, Lmax):
    """Per-utterance lengths (a list or an integer tensor, read once, here; None: every utterance is Lmax long) -> a list of B ints"""
    if lengths is None:
        return [int(Lmax)] * B
    lengths = [int(v) for v in (lengths.reshape(-1).tolist() if _is_tensor(lengths) else lengths)]
    if len(lengths) != B or min(lengths) < 1 or max(lengths) > Lmax:
        raise ValueError(f"lengths must be {B} values in [1, {Lmax}], got {lengths}")
    return lengths


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def _chunk(L, flag, Ks):
    """One utterance of L samples in half-overlapping segments of Ks (utility.py:327-329, 360-368): a reset (flag clear) leads with
    P = Ks / 2 zeros and strips them again.  -> (Lp, gap, number of segments, first segment's start sample, samples stripped)"""
    P = Ks // 2
    lead = 0 if flag else P
    Lp = L + lead
    gap = Ks - (P + Lp % Ks) % Ks
    return Lp, gap, 2 * (Lp + gap + P) // Ks, -P - lead, lead


def segment_geometry(L, flag, segment_length, hop, n_fft, ch=()):
    """One realtime_process call over L samples in half-overlapping segments (utility.segmentation); flag=False pads P = Ks / 2 samples
    on the left and strips them again.  ch = the U-Net levels' channels, input first; Fq[i] = level i's frequency size (stride 2)."""
    Ks = segment_length
    Lp, gap, N, off0, skip = _chunk(L, flag, Ks)
    Fq = [n_fft // 2 + 1]
    for _ in ch[1:]:
        Fq.append((Fq[-1] - 1) // 2 + 1)
    return dict(L=L, Ks=Ks, P=Ks // 2, Lp=Lp, gap=gap, N=N, off0=off0, skip=skip, T=1 + Ks // hop, F0=Fq[0], ch=list(ch), Fq=Fq)


def ragged_geometry(lengths, flags, segment_length, hop, n_fft, ch=()):
    """A batch of chunk chains in one call: utterance b is lengths[b] samples long and continues its own state iff flags[b].  Segment
    positions do not depend on the length, so every utterance keeps the geometry it would have alone: Lp, gap, Nb, off0, skip are lists,
    entry b = segment_geometry(lengths[b], flags[b], ...); N = max Nb segments are run, L = max length is the width of the batch."""
    per = [segment_geometry(int(L), bool(f), segment_length, hop, n_fft, ch) for L, f in zip(lengths, flags)]
    q = dict(per[0])
    q.update(L=max(p["L"] for p in per), N=max(p["N"] for p in per), lengths=[p["L"] for p in per], flags=[bool(f) for f in flags],
             Nb=[p["N"] for p in per], **{k: [p[k] for p in per] for k in ("Lp", "gap", "off0", "skip")})
    return q


def chain_geometry(lengths, flags, segment_length):
    """Per-stream segment geometry of one se_realtime_process_chains call: Nb[b] segments, the first one starting at sample off0[b] of
    the stream, skip[b] samples stripped from its overlap-average; the call runs N = max Nb segments.  What the engines' chunk_geometry
    (csrc/chain_plan.h, exported as se_chunk_geometry) computes, and ragged_geometry without the STFT sizes."""
    per = [_chunk(int(L), f, int(segment_length)) for L, f in zip(lengths, flags)]
    Nb = [p[2] for p in per]
    return dict(Nb=Nb, off0=[p[3] for p in per], skip=[p[4] for p in per], N=max(Nb) if Nb else 0)


# ---- the plan --------------------------------------------------------------------------------------------------------------------
class CallPlan:
    """One call over B utterances of up to L samples.  `geo` is segment_geometry's dict (uniform) or ragged_geometry's (chains), and its
    entries are attributes too: Ks, P, T, F0, ch, Fq, N, and off0 / skip / Lp / gap - ints when uniform, lists of B when not.  Whatever
    the kind: flags, lengths, Nb (lists of B), any_flag, flag (the one flag of a uniform call), L (the batch width).  `rows`: the caller's
    row of every utterance - the identity, unless the plan is a part of a call (streaming.StreamingMixin._prefix_passes).  `dev` is
    train_stages.row_table's cache of device tables.  uniform=False forces the chains form on a batch that would triage as uniform."""

    def __init__(self, flags, lengths, L, segment_length, hop, n_fft, ch=(), uniform=None):
        if uniform is None:
            uniform = len(set(flags)) == 1 and min(lengths) == L
        self.geo = (segment_geometry(L, flags[0], segment_length, hop, n_fft, ch) if uniform else
                    ragged_geometry(lengths, flags, segment_length, hop, n_fft, ch))
        self.__dict__.update(self.geo)
        self.uniform, self.B, self.L = uniform, len(flags), L
        self.flags, self.lengths, self.any_flag, self.flag = list(flags), list(lengths), any(flags), flags[0] if uniform else None
        self.Nb = self.geo.get("Nb", [self.N] * self.B)
        self.rows = list(range(self.B))
        self.dev = {}

    def table(self, key):
        """Host values of what the `_rows` kernels index by utterance (chains): off0 / len / skip, `last` = the slab after utterance b's
        own last segment, `lastseg` = that segment, `carry` = 0 where utterance b continues its carried row, -1 (zeros) where it starts"""
        return dict(off0=self.off0, len=self.lengths, skip=self.skip, last=self.Nb, lastseg=[n - 1 for n in self.Nb],
                    carry=[0 if f else -1 for f in self.flags])[key]

    def live(self, n0=0, Nc=None):
        """per utterance: how many of the segments [n0, n0 + Nc) are its own"""
        return [min(max(nb - n0, 0), self.N - n0 if Nc is None else Nc) for nb in self.Nb]


def call_plan(flag, lengths, B, Lmax, segment_length, hop, n_fft, ch=(), uniform=None):
    """The CallPlan of realtime_process(mixture [B, M, Lmax], flag, lengths): parse, validate, triage (unless `uniform` decides)."""
    return CallPlan(as_flags(flag, B), as_lengths(lengths, B, Lmax), Lmax, segment_length, hop, n_fft, ch, uniform)


def chain_passes(Nb_sorted, step):
    """The passes of a chunk-chain call whose streams are sorted by window count, descending: [(n0, Nc, Bp), ...] - windows
    [n0, n0 + Nc) of the call, run on the Bp leading streams, the ones with a window of their own at n0 or later."""
    N, step = max(Nb_sorted, default=0), max(1, int(step))
    return [(n0, min(step, N - n0), sum(nb > n0 for nb in Nb_sorted)) for n0 in range(0, N, step)]


# ---- signal glue of the torch restatements (utility.py:312-403): differentiable, dtype-generic -----------------------------------
def windows(plan, x):
    """x [B, C, L] -> the plan's N half-overlapping windows of every utterance's own samples [B, C, N, Ks]: utterance b is
    x[b, :, :lengths[b]], window n starts at sample off0[b] + n * P, zeros outside."""
    import torch
    import torch.nn.functional as Fn
    N, P, Ks = plan.N, plan.P, plan.Ks
    if plan.uniform:
        xp = Fn.pad(x, (-plan.off0, (N + 1) * P + plan.off0 - plan.L))
    else:
        xp = torch.cat([Fn.pad(x[b:b + 1, :, :L], (-o, (N + 1) * P + o - L)) for b, (L, o) in enumerate(zip(plan.lengths, plan.off0))])
    idx = (torch.arange(N, device=x.device) * P)[:, None] + torch.arange(Ks, device=x.device)[None, :]
    return xp[:, :, idx]


def overlap_add_cut(plan, y):
    """y [B, N, Ks] -> [B, L]: utility.over_add (the average of the even and the odd windows' streams), then every utterance's own
    samples - the lead of a reset and the gap dropped - with zeros beyond its length."""
    import torch
    import torch.nn.functional as Fn
    B, P = y.shape[0], plan.P
    full = (y[:, 0::2].reshape(B, -1)[:, P:] + y[:, 1::2].reshape(B, -1)[:, :-P]) / 2
    if plan.uniform:
        return full[:, plan.skip:plan.skip + plan.L]
    return torch.stack([Fn.pad(full[b, s:s + L], (0, plan.L - L)) for b, (L, s) in enumerate(zip(plan.lengths, plan.skip))])


def _hamming(win, like, dtype):
    import torch
    return torch.hamming_window(win, device=like.device, dtype=dtype)


def stft_windows(seg, n_fft, hop, win, window_dtype):
    """stft_trans of windows [..., Ks] -> complex [..., F, T] (torch.stft as speechbrain's STFT wrapper calls it).  window_dtype: the
    Hamming window's - the drop-in models take the input's, the training restatements float32 whatever the input is."""
    import torch
    X = torch.stft(seg.reshape(-1, seg.shape[-1]), n_fft, hop, win, _hamming(win, seg, window_dtype), center=True, pad_mode="constant",
                   normalized=False, onesided=True, return_complex=True)
    return X.reshape(*seg.shape[:-1], *X.shape[-2:])


def istft_windows(spec, n_fft, hop, win, window_dtype):
    """complex [..., F, T] -> windows [..., Ks], the inverse of stft_windows"""
    import torch
    y = torch.istft(spec.reshape(-1, *spec.shape[-2:]), n_fft, hop, win, _hamming(win, spec, window_dtype), center=True, normalized=False,
                    onesided=True)
    return y.reshape(*spec.shape[:-2], y.shape[-1])
