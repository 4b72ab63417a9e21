"""call_plan.py, the one home of flag / lengths parsing, the segment geometry and the triage of a realtime_process call: the CallPlan
against segment_geometry / ragged_geometry field by field, the parser names the other modules keep, and the restatements' signal glue
(windows, overlap_add_cut) of a chains plan against uniform plans of every utterance alone.  No library, no GPU."""
import numpy as np
import pytest
import torch

from speech_enhancement_mi_amd import call_plan as cp

KS, HOP, NFFT, CH = 3200, 160, 400, [5, 16, 32]
LMAX = 8000
ROW_LENS, ROW_FLAGS = (8000, 5200, 3400, 1), (False, True, False, True)   # the rows of tests/test_gpu_chain_training.py


def _lists():
    """the length and flag lists of test_chain_cpu.py::test_ragged_geometry_is_segment_geometry_per_utterance"""
    rng = np.random.default_rng(0)
    lengths = [1, 799, 1599, 1600, 1601, 3199, 3200, 3201, 4800, 4801, 16000, 59999] + [int(v) for v in rng.integers(1, 60000, 40)]
    return lengths, [bool(v) for v in rng.integers(0, 2, len(lengths))]


@pytest.mark.parametrize("flag", [False, True])
def test_one_flag_and_full_lengths_give_a_uniform_plan(flag):
    B = 3
    want = cp.segment_geometry(LMAX, flag, KS, HOP, NFFT, CH)
    forms = [flag, int(flag), torch.tensor(flag), torch.tensor([flag]), [flag], [flag] * B, (flag,) * B, torch.tensor([flag] * B)]
    for form in forms:
        for lengths in (None, [LMAX] * B, torch.tensor([LMAX] * B)):
            p = cp.call_plan(form, lengths, B, LMAX, KS, HOP, NFFT, CH)
            assert p.uniform and p.geo == want and p.flag is flag and p.any_flag is flag, (form, lengths)
            assert all(getattr(p, k) == v for k, v in want.items())
            assert (p.B, p.L, p.flags, p.lengths, p.Nb) == (B, LMAX, [flag] * B, [LMAX] * B, [want["N"]] * B)


def test_mixed_flags_or_a_shorter_length_give_a_chains_plan():
    lengths, flags = _lists()
    B, Lmax = len(lengths), max(lengths) + 7
    for Ks, hop, n_fft in ((3200, 160, 400), (3200, 160, 512), (1600, 160, 400)):
        p = cp.call_plan(torch.tensor(flags), torch.tensor(lengths), B, Lmax, Ks, hop, n_fft, CH)
        want = cp.ragged_geometry(lengths, flags, Ks, hop, n_fft, CH)
        assert not p.uniform and p.geo == want and p.flag is None and p.any_flag
        assert all(getattr(p, k) == v for k, v in want.items() if k != "L") and p.L == Lmax   # L: the width of the batch, not the longest
        assert p.table("len") == lengths and p.table("last") == want["Nb"] and p.table("lastseg") == [n - 1 for n in want["Nb"]]
        assert p.table("carry") == [0 if f else -1 for f in flags] and p.table("off0") == want["off0"] and p.table("skip") == want["skip"]
    for form, lens in (([False, True, False], None), (False, [LMAX, LMAX - 1, LMAX]), ([True], [1, LMAX, LMAX])):
        p = cp.call_plan(form, lens, 3, LMAX, KS, HOP, NFFT)
        fl, ln = cp.as_flags(form, 3), cp.as_lengths(lens, 3, LMAX)
        assert not p.uniform and p.geo == cp.ragged_geometry(ln, fl, KS, HOP, NFFT) and (p.flags, p.lengths) == (fl, ln)
    forced = cp.call_plan(True, None, 2, LMAX, KS, HOP, NFFT, uniform=False)   # the chains form of a uniform batch
    assert not forced.uniform and forced.geo == cp.ragged_geometry([LMAX] * 2, [True] * 2, KS, HOP, NFFT)


def test_live_segments_of_a_pass():
    p = cp.call_plan(ROW_FLAGS, ROW_LENS, 4, LMAX, KS, HOP, NFFT)
    assert p.Nb == [8, 6, 6, 2] and p.N == 8
    assert p.live() == p.Nb and p.live(0, 3) == [3, 3, 3, 2] and p.live(3, 3) == [3, 3, 3, 0] and p.live(6, 2) == [2, 0, 0, 0]


def test_bad_arguments_raise_where_they_are_parsed():
    for bad, frag in (([True, False], "2 flags for a batch of 3 utterances"), (torch.tensor([1, 0, 1, 1]), "4 flags for a batch of 3")):
        with pytest.raises(ValueError, match=frag):
            cp.call_plan(bad, None, 3, LMAX, KS, HOP, NFFT)
    for bad in ([LMAX, LMAX], [LMAX, LMAX + 1, 5], [LMAX, 0, 5]):
        with pytest.raises(ValueError, match="lengths must be 3 values in"):
            cp.call_plan(False, bad, 3, LMAX, KS, HOP, NFFT)


def test_the_old_parser_names_are_forms_of_the_one_parser():
    from speech_enhancement_mi_amd import engine, train_stages as ts
    assert engine._flags_of is cp.flags_of and engine.chain_geometry is cp.chain_geometry
    assert ts.segment_geometry is cp.segment_geometry and ts.ragged_geometry is cp.ragged_geometry
    f = engine._flags_of
    assert f(True, 3) is True and f(0, 3) is False and f(torch.tensor([True]), 3) is True and f([1], 3) is True
    assert f(torch.tensor([1, 0, 1]), 3) == [True, False, True] and f((0, 1), 2) == [False, True]
    with pytest.raises(RuntimeError, match="2 flags for a batch of 3$"):
        f([True, False], 3)
    assert ts._as_flag(True) is True and ts._as_flag(0) is False and ts._as_flag(torch.tensor([True, False])) is True
    assert ts._as_flags(torch.tensor([True, False, True]), 3) == [True, False, True] and ts._as_flags(torch.tensor(False), 1) == [False]
    assert ts._as_flags(True, 2) == [True, True] and ts._as_flags([1], 2) == [True, True] and ts._as_flags([0, 1], 2) == [False, True]
    with pytest.raises(ValueError, match="3 flags for a batch of 2 utterances"):
        ts._as_flags([True, False, True], 2)
    assert ts._as_lengths(None, 2, 7) == [7, 7] and ts._as_lengths(torch.tensor([3, 7]), 2, 7) == [3, 7] and ts._as_lengths((1, 2), 2, 7) == [1, 2]
    for bad in ([3], [3, 8], [0, 7]):
        with pytest.raises(ValueError, match=r"lengths must be 2 values in \[1, 7\], got"):
            ts._as_lengths(bad, 2, 7)


def test_chain_geometry_is_ragged_geometry_without_the_stft_sizes():
    lengths, flags = _lists()
    for Ks in (3200, 1600):
        q, g = cp.ragged_geometry(lengths, flags, Ks, HOP, NFFT), cp.chain_geometry(lengths, flags, Ks)
        assert g == dict(Nb=q["Nb"], off0=q["off0"], skip=q["skip"], N=q["N"])
    assert cp.chain_geometry([], [], KS)["N"] == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_glue_of_a_chains_plan_is_every_utterance_alone(dtype):
    """windows and overlap_add_cut of utterance b in the batch == those of a uniform plan built for utterance b alone, exactly; what lies
    beyond an utterance's length is neither read nor written."""
    B = len(ROW_LENS)
    torch.manual_seed(0)
    x = torch.randn(B, 2, LMAX, dtype=dtype)
    p = cp.call_plan(ROW_FLAGS, ROW_LENS, B, LMAX, KS, HOP, NFFT)
    w = cp.windows(p, x)
    assert w.shape == (B, 2, p.N, KS) and w.dtype == dtype
    y = torch.randn(B, p.N, KS, dtype=dtype)
    out = cp.overlap_add_cut(p, y)
    assert out.shape == (B, LMAX) and out.dtype == dtype
    for b, (L, f) in enumerate(zip(ROW_LENS, ROW_FLAGS)):
        one = cp.call_plan(f, None, 1, L, KS, HOP, NFFT)
        assert one.uniform and one.N == p.Nb[b]
        assert torch.equal(w[b:b + 1, :, :one.N], cp.windows(one, x[b:b + 1, :, :L].contiguous())), b
        assert not w[b, :, one.N:].any(), "windows past an utterance's own last one are silent"
        assert torch.equal(out[b:b + 1, :L], cp.overlap_add_cut(one, y[b:b + 1, :one.N])), b
        assert not out[b, L:].any()


@pytest.mark.parametrize("flag", [False, True])
def test_overlap_add_of_the_windows_returns_the_signal(flag):
    """The even windows tile the padded signal from sample 0, the odd ones from sample P, and over_add averages the two streams where
    both exist - which is everywhere between the lead and the gap.  Of plain windows both streams hold the same samples, so (x + x) / 2
    gives the signal back exactly, over the whole utterance and therefore away from its first and last half segment too; uniform and
    chains, and the gradient of the sum is one per own sample."""
    x = torch.randn(2, 1, LMAX, dtype=torch.float64, requires_grad=True)
    for p in (cp.call_plan(flag, None, 2, LMAX, KS, HOP, NFFT), cp.call_plan(flag, [LMAX, 5000], 2, LMAX, KS, HOP, NFFT)):
        back = cp.overlap_add_cut(p, cp.windows(p, x)[:, 0])
        for b, L in enumerate(p.lengths):
            assert torch.equal(back[b, :L], x[b, 0, :L]), (flag, b)
            assert not back[b, L:].any()
        grad, = torch.autograd.grad(back.sum(), x)
        for b, L in enumerate(p.lengths):
            assert torch.equal(grad[b, 0, :L], torch.ones(L, dtype=x.dtype)) and not grad[b, 0, L:].any()
