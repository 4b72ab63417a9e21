"""Batched chunk-chain training on the kernels (per-utterance lengths and flags): the row kernels against per-utterance launches of the
scalar ones, bit for bit; the kernel path against what the genuine reference gives for every utterance alone
(tests/golden/crn_chain_golden.npz); and the batched call against the utterances run one by one on the same kernels."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from chain_cases import CALLS, VARIANTS, chain_batch, chain_golden, tiny_model
from conftest import FULL400, TINY, rel_rms, spec_of
from speech_enhancement_mi_amd import synth

pytestmark = pytest.mark.gpu

# Batched-vs-alone relative error of pred for a UNIFORM batch (4 x 9600 samples, reset call and continuation; runs on the parent commit
# too), measured on an MI355X: utterance b of a batch goes through the same kernels with the same per-stream arithmetic as alone, and
# the figure came out as exactly 0 (bit-identical rows).  The ragged case is allowed twice that figure - bit equality - plus nothing.
PRED_UNIFORM = 0.0
PRED_BOUND = 2.0 * PRED_UNIFORM
GRAD_BOUND = 2e-5   # test_gpu_round3.py::test_merged_microbatches_give_the_accumulated_gradient, the same kind of regrouping


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _i64(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def _sig():
    from speech_enhancement_mi_amd import train_net as N
    return N._sig(torch.device("cuda", 0), 400, 400, 160, 3200)


ROW_LENS, ROW_FLAGS, ROW_LMAX = (8000, 5200, 3400, 1), (False, True, False, True), 8000


def test_stft_rows_equals_the_scalar_kernel_per_utterance():
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.train_stages import ragged_geometry
    lib, sig = K._lib(), _sig()
    q = ragged_geometry(ROW_LENS, ROW_FLAGS, 3200, 160, 400)
    B, M, N, P = len(ROW_LENS), 3, q["N"], q["P"]
    x = torch.randn(B, M, ROW_LMAX, device="cuda")   # "padding" = noise: the kernel must cut it off itself
    spec = torch.full((N, B * M, 21, 201, 2), 7.0, device="cuda")
    off0, lens = _i64(q["off0"]), _i64(ROW_LENS)
    K._chk(lib.se_sig_stft_rows(sig, _vp(x), B, M, ROW_LMAX, _vp(off0), _vp(lens), P, N, _vp(spec), K._st()))
    for b, L in enumerate(ROW_LENS):
        xb = x[b:b + 1].clone()
        xb[..., L:] = 0
        one = torch.empty(N, M, 21, 201, 2, device="cuda")
        K._chk(lib.se_sig_stft(sig, _vp(xb), 1, M, ROW_LMAX, q["off0"][b], P, N, _vp(one), K._st()))
        assert torch.equal(spec[:, b * M:(b + 1) * M], one), b
        assert not spec[q["Nb"][b]:, b * M:(b + 1) * M].any(), "segments past an utterance's end are silent"


def test_ola_rows_equal_the_scalar_kernels_per_utterance():
    from speech_enhancement_mi_amd import train_ops as K
    from speech_enhancement_mi_amd.train_stages import ragged_geometry
    lib, sig = K._lib(), _sig()
    q = ragged_geometry(ROW_LENS, ROW_FLAGS, 3200, 160, 400)
    B, N, Ks = len(ROW_LENS), q["N"], 3200
    skip, lens = _i64(q["skip"]), _i64(ROW_LENS)
    yseg = torch.randn(N, B, Ks, device="cuda")
    out = torch.full((B, ROW_LMAX), 7.0, device="cuda")
    K._chk(lib.se_train_ola_fwd_rows(sig, _vp(yseg), _vp(out), B, ROW_LMAX, _vp(skip), _vp(lens), K._st()))
    dout = torch.randn(B, ROW_LMAX, device="cuda")
    gseg = torch.full((N, B, Ks), 7.0, device="cuda")
    K._chk(lib.se_train_ola_bwd_rows(sig, _vp(dout), _vp(gseg), B, N, ROW_LMAX, _vp(skip), _vp(lens), K._st()))
    for b, L in enumerate(ROW_LENS):
        yb = yseg[:, b:b + 1].contiguous()
        ob = torch.empty(1, L, device="cuda")
        K._chk(lib.se_train_ola_fwd(sig, _vp(yb), _vp(ob), 1, L, q["skip"][b], K._st()))
        assert torch.equal(out[b, :L], ob[0]) and not out[b, L:].any(), b
        db = dout[b:b + 1, :L].contiguous()
        gb = torch.empty(N, 1, Ks, device="cuda")
        K._chk(lib.se_train_ola_bwd(sig, _vp(db), _vp(gb), 1, N, L, q["skip"][b], K._st()))
        assert torch.equal(gseg[:, b], gb[:, 0]), b
    dirty = dout.clone()
    for b, L in enumerate(ROW_LENS):
        dirty[b, L:] = float("nan")
    g2 = torch.empty_like(gseg)
    K._chk(lib.se_train_ola_bwd_rows(sig, _vp(dirty), _vp(g2), B, N, ROW_LMAX, _vp(skip), _vp(lens), K._st()))
    assert torch.equal(g2, gseg), "the adjoint must not read dout[b, L_b:]"


def test_slab_gather():
    from speech_enhancement_mi_amd.train_stages import slab_gather
    N, B, X = 5, 4, 1000
    src = torch.randn(N + 1, B, X, device="cuda")
    idx = [5, 2, -1, 0]
    dst = slab_gather(src, _i64(idx), B, X, B * X, X)
    for b, n in enumerate(idx):
        assert torch.equal(dst[b], src[n, b]) if n >= 0 else not dst[b].any()
    part = slab_gather(src, _i64([4, 1, 3, -1]), B, 10, B * X, X, off_floats=X - 10)   # the last 10 floats of a row
    for b, n in enumerate([4, 1, 3, -1]):
        assert torch.equal(part[b], src[n, b, -10:]) if n >= 0 else not part[b].any()


@pytest.mark.parametrize("tag,variant", VARIANTS)
def test_kernel_path_batched_chains_match_the_reference_per_utterance(tag, variant):
    """test_chain_cpu.py's fixture case on the kernels: 1e-4 relative RMS per utterance and call, nothing beyond an utterance's length"""
    g = chain_golden()
    m = tiny_model(variant).cuda().use_hip_kernels(True)
    with torch.no_grad():
        for c, (flags, lens) in enumerate(CALLS):
            pred = m.realtime_process_train(chain_batch(c).cuda(), torch.tensor(flags), lengths=list(lens))
            for b, L in enumerate(lens):
                err = rel_rms(pred[b, :L].cpu().numpy(), g[f"{tag}_call{c + 1}_utt{b}"])
                print(f"{tag} call {c + 1} utterance {b}: rel rms {err:.2e}")
                assert err < 1e-4, (tag, c, b, err)
                assert not pred[b, L:].any()


def _full_model(seed=2):
    from speech_enhancement_mi_amd.training import TrainableCRN
    m = TrainableCRN(**FULL400)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec_of(FULL400), seed=seed).items()})
    return m.cuda().use_hip_kernels(True)


def _flat_grad(m):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()])


def test_uniform_batch_is_unchanged():
    """flag as a uniform tensor + lengths = [L] * B is the bool call, bit for bit - through the dispatch (scalar kernels) and when the
    row kernels themselves are given the uniform batch; a reset call and a continuation, pred and every gradient."""
    from speech_enhancement_mi_amd.train_net import CRNFunction, _plan
    B, L = 4, 6400
    mix, _ = synth.synth_utterances(B, 2 * L, 3, seed=31)
    x = torch.from_numpy(mix).cuda()
    w = torch.randn(B, L, device="cuda")
    res = {}
    for how in ("bool", "uniform", "rows"):
        m = _full_model()
        out = []
        for c, flag in enumerate((False, True)):
            xc = x[..., c * L:(c + 1) * L].contiguous()
            if how == "bool":
                pred = m.realtime_process_train(xc, flag)
            elif how == "uniform":
                pred = m.realtime_process_train(xc, torch.tensor([flag] * B), lengths=[L] * B)
            else:
                pred = CRNFunction.apply(m, xc, _plan(m, xc, flag, uniform=False), *[p for _, p in m.named_parameters()])
            m.zero_grad()
            (pred * w).sum().backward()
            out += [pred.detach().clone(), _flat_grad(m).clone()]
        res[how] = out
    for how in ("uniform", "rows"):
        for a, b in zip(res[how], res["bool"]):
            assert torch.equal(a, b), how


# four chains, two steps; every utterance has at least four segments in both calls, like the uniform measurement
BA_CALLS = (((False, False, False, False), (16000, 11000, 7300, 5000)), ((True, False, True, True), (6000, 12000, 9000, 4000)))
BA_UNIFORM = (((False,) * 4, (9600,) * 4), ((True,) * 4, (9600,) * 4))


def _batched_vs_alone(calls, seed):
    """-> per call: [pred error per utterance], gradient error, [state error per utterance]; the full loss (0.7 STOI + 0.3 -SI-SNR) is a
    mean over the batch, so the batched gradient is the mean of the alone-runs' gradients"""
    B = len(calls[0][1])
    total = max(calls[0][1]) + max(calls[1][1])
    mix, clean = synth.synth_utterances(B, total, 3, seed=seed)

    def batch(c, rows, arr):
        lens = [calls[c][1][b] for b in rows]
        out = np.zeros((len(rows),) + arr.shape[1:-1] + (max(calls[c][1]) if len(rows) > 1 else lens[0],), np.float32)
        for i, b in enumerate(rows):
            lo = 0 if c == 0 else calls[0][1][b]
            out[i, ..., :lens[i]] = arr[b, ..., lo:lo + lens[i]]
        return torch.from_numpy(out).cuda()

    def run(rows):
        m = _full_model(seed=4)
        res = []
        for c, (flags, lens) in enumerate(calls):
            ln = torch.tensor([lens[b] for b in rows], device="cuda")
            x, src = batch(c, rows, mix), batch(c, rows, clean)
            if len(rows) > 1:
                pred = m.realtime_process_train(x, torch.tensor([flags[b] for b in rows]), lengths=ln)
            else:
                pred = m.realtime_process_train(x, flags[rows[0]])
            m.zero_grad()
            m.compute_loss(src, pred, ln)[0].backward()
            st = m._state
            flat_state = torch.cat([t.reshape(len(rows), -1) for t in st["buf"] + list(st["h"])], dim=1)
            res.append((pred.detach().clone(), _flat_grad(m).clone(), flat_state.clone()))
        return res

    both = run(list(range(B)))
    alone = [run([b]) for b in range(B)]
    out = []
    for c, (flags, lens) in enumerate(calls):
        pe = [_rel(both[c][0][b, :lens[b]], alone[b][c][0][0]) for b in range(B)]
        assert all(not both[c][0][b, lens[b]:].any() for b in range(B))
        ge = _rel(both[c][1], sum(alone[b][c][1] for b in range(B)) / B)
        se = [_rel(both[c][2][b], alone[b][c][2][0]) for b in range(B)]
        out.append((pe, ge, se))
    return out


def test_batched_chains_match_the_utterances_run_alone():
    """FULL400, four chains, two calls with mixed flags and lengths: per-utterance pred and carried state within PRED_BOUND of the
    utterance run alone, the flat gradient of the full loss within GRAD_BOUND of the alone-runs' (the figures are printed first; the
    uniform batch - which the parent commit runs too - is measured alongside and must not have moved from PRED_UNIFORM)."""
    uni = _batched_vs_alone(BA_UNIFORM, seed=41)
    rag = _batched_vs_alone(BA_CALLS, seed=43)
    for name, res in (("uniform", uni), ("ragged", rag)):
        for c, (pe, ge, se) in enumerate(res):
            print(f"{name} call {c + 1}: pred {max(pe):.3e} state {max(se):.3e} gradient {ge:.3e}")
    assert max(max(pe) for pe, _, _ in uni) <= PRED_UNIFORM, "re-measure PRED_UNIFORM"
    for pe, ge, se in rag:
        assert max(pe) <= PRED_BOUND, pe
        assert max(se) <= PRED_BOUND, se
        assert ge < GRAD_BOUND, ge


def test_chain_gradients_are_bit_reproducible():
    runs = []
    for _ in range(2):
        m = tiny_model(1).cuda().use_hip_kernels(True)
        out = []
        for c, (flags, lens) in enumerate(CALLS):
            pred = m.realtime_process_train(chain_batch(c).cuda(), list(flags), lengths=list(lens))
            m.zero_grad()
            (pred ** 2).sum().backward()
            out += [pred.detach().clone(), _flat_grad(m).clone()]
        runs.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_train_step_with_lengths_and_flags_merged_and_sequential():
    """train_step(length=, flag=) with loss="full", accum=2: one merged sweep against the sequential micro-batches, the bounds of
    test_merged_microbatches_give_the_accumulated_gradient; then a second, mixed-flag step on the merged model stays finite."""
    from speech_enhancement_mi_amd.training import FlatBucket, train_step
    flags, lens = BA_CALLS[0]
    mix, clean = synth.synth_utterances(4, max(lens), 3, seed=87)
    x, c = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()
    ln = torch.tensor(lens, device="cuda")
    res = {}
    for merge in (True, False):
        m = _full_model(seed=4)
        bucket = FlatBucket(list(m.parameters()))
        opt = torch.optim.Adam(m.parameters(), lr=3e-4)
        l = train_step(m, bucket, opt, x, c, ln, accum=2, loss="full", merge=merge, flag=torch.tensor(flags))
        res[merge] = (l, bucket.flat.clone(), torch.cat([p.detach().flatten() for p in m.parameters()]))
        if merge:
            l2 = train_step(m, bucket, opt, x[..., :12000].contiguous(), c[:, :12000].contiguous(), torch.tensor(BA_CALLS[1][1], device="cuda"), accum=2,
                            loss="full", flag=torch.tensor(BA_CALLS[1][0]))
            assert np.isfinite(l2) and bool(torch.isfinite(bucket.flat).all())
    assert abs(res[True][0] - res[False][0]) < 1e-5 * max(1.0, abs(res[False][0]))
    assert _rel(res[True][1], res[False][1]) < 2e-5
    assert _rel(res[True][2], res[False][2]) < 1e-6


def test_distillation_forward_with_per_utterance_flags_and_lengths(tmp_path):
    """DistillationCRN.forward on a batch of chunk chains.  STOI and SI-SNR are means over the batch: against the utterances run one by
    one.  The feature loss is not a sum over utterances (BatchNorm statistics and the mean run over all windows of the batch), so the
    total loss is compared with the torch restatement of the same batched call instead; tolerance: test_gpu_distill.py's loss bar, 2e-4."""
    from test_gpu_distill import _train_setup
    base = _train_setup(tmp_path, TINY, seed=3)
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    _, clean = synth.synth_utterances(3, 12800, 3, seed=21)

    def src(c, rows):
        lens = CALLS[c][1]
        out = np.zeros((len(rows), max(lens) if len(rows) > 1 else lens[rows[0]]), np.float32)
        for i, b in enumerate(rows):
            lo = 0 if c == 0 else CALLS[0][1][b]
            out[i, :lens[b]] = clean[b, lo:lo + lens[b]]
        return torch.from_numpy(out).cuda()

    def run(hip, rows):
        m = _train_setup(tmp_path, TINY, seed=3)
        m.load_state_dict(sd)
        m = m.cuda().use_hip_kernels(hip)
        out = []
        with torch.no_grad():
            for c, (flags, lens) in enumerate(CALLS):
                x = chain_batch(c).cuda()
                if len(rows) == 1:
                    b = rows[0]
                    x = x[b:b + 1, :, :lens[b]].contiguous()
                out.append([float(v) for v in m(x, src(c, rows), torch.tensor([lens[b] for b in rows], device="cuda"), torch.tensor([flags[b] for b in rows]))])
        return out

    hip, ref = run(True, [0, 1, 2]), run(False, [0, 1, 2])
    alone = [run(True, [b]) for b in range(3)]
    for c in range(2):
        print(f"call {c + 1}: kernels {hip[c]} restatement {ref[c]} alone {[a[c] for a in alone]}")
        assert abs(hip[c][0] - ref[c][0]) < 2e-4 * max(1.0, abs(ref[c][0]))
        for k in (1, 2):
            mean = sum(a[c][k] for a in alone) / 3
            assert abs(hip[c][k] - mean) < 2e-4 * max(1.0, abs(mean)), (c, k, hip[c][k], mean)
