"""FullSubNet training on the MI355X: TrainableFullSubNet(...).use_hip_kernels(True) (fsn_train_fwd / fsn_train_bwd: the LSTM
backward k_lstm_bwd_step and its companions, csrc/fsn_train.hip.h) against the reference's gradients (tiny configuration) and
against the torch-autograd restatement (full configuration), plus the reference trainer's loop (train_fullsubnet.py:137-145)."""
import os

import numpy as np
import pytest
import torch

from conftest import FSN_FULL, FSN_TINY, ROOT, fsn_spec, rel_rms

pytestmark = pytest.mark.gpu

CHUNKS = ((0, 4800, False), (4800, 8000, True))


def _sd(cfg, seed):
    from speech_enhancement_mi_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(fsn_spec(cfg), seed=seed).items()}


def _model(cfg, sd, hip, dtype=torch.float32):
    from speech_enhancement_mi_amd.fsn_training import TrainableFullSubNet
    m = TrainableFullSubNet(**cfg)
    m.load_state_dict(sd)
    return m.cuda().to(dtype).use_hip_kernels(hip)


def _flat(m):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in m.parameters()]).detach().clone()


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_hip_vs_reference_gradients_tiny():
    from speech_enhancement_mi_amd import synth
    gg = np.load(os.path.join(ROOT, "tests", "golden", "fsn_grad_golden.npz"))
    m = _model(FSN_TINY, _sd(FSN_TINY, 0), True)
    mix, clean = synth.synth_utterances(2, 8000, 3, seed=7)
    src = np.repeat(clean[:, None, :], 3, axis=1)
    for c, (a, b, flag) in enumerate(CHUNKS):
        m.zero_grad(set_to_none=True)
        pred = m.realtime_process(torch.from_numpy(mix[..., a:b]).cuda(), torch.from_numpy(src[..., a:b]).cuda(), flag=flag, train=False)[0]
        assert rel_rms(pred.detach().cpu().numpy(), gg[f"c{c}_pred"]) <= 1e-4
        (pred * torch.from_numpy(gg[f"c{c}_R"]).cuda()).sum().backward()
        for k, p in m.named_parameters():
            e = rel_rms(p.grad.cpu().numpy(), gg[f"c{c}_grad.{k}"])
            print(f"chunk {c} {k}: {e:.2e}")
            assert e <= 1e-3, f"chunk {c} {k}: rel rms {e:.2e}"


def test_hip_full_config_vs_float64_restatement():
    """FSN_FULL (512 / 384), 2 x 1.5 s, MSE loss: the kernels must be as close to float64 autograd as torch's own fp32 is (the floor
    rule of test_fused_train_step_at_bench_shape_vs_torch_autograd), for the flat gradient AND for every parameter tensor on its own
    (the full-band gradients are orders of magnitude smaller than the sub-band ones: an error confined to them would vanish in the
    flat norm)."""
    from speech_enhancement_mi_amd import synth
    sd = _sd(FSN_FULL, 3)
    mix, clean = synth.synth_utterances(2, 24000, 3, seed=91)
    x, c = torch.from_numpy(mix).cuda(), torch.from_numpy(clean).cuda()

    def run(hip, dtype):
        m = _model(FSN_FULL, sd, hip, dtype)
        pred = m.realtime_process(x.to(dtype), flag=False, train=False)
        (((pred - c.to(dtype)) ** 2).mean() * 100.0).backward()
        return {k: p.grad.detach().double().clone() for k, p in m.named_parameters()}

    g64, gt, gh = run(False, torch.float64), run(False, torch.float32), run(True, torch.float32)
    flat = lambda g: torch.cat([v.flatten() for v in g.values()])
    e_t, e_h = _rel(flat(gt), flat(g64)), _rel(flat(gh), flat(g64))
    print(f"flat-gradient error vs float64 autograd: torch fp32 {e_t:.2e}, HIP kernels {e_h:.2e}")
    assert e_h <= max(2.0 * e_t, 5e-5), (e_h, e_t)
    bad = []
    for k in g64:
        assert float(g64[k].norm()) > 0, k
        et, eh = _rel(gt[k], g64[k]), _rel(gh[k], g64[k])
        print(f"{k}: |g| {float(g64[k].norm()):.2e}  torch fp32 {et:.2e}  HIP {eh:.2e}")
        if eh > max(2.0 * et, 5e-5):
            bad.append((k, eh, et))
    assert not bad, bad


def test_hip_training_microbatch_full_loss_and_reproducible():
    """8 x 3 s (the training micro-batch), full compute_loss: loss and flat gradient against the torch fp32 restatement on the same
    GPU, and two HIP runs give identical gradients (no float atomics)."""
    from speech_enhancement_mi_amd import synth
    sd = _sd(FSN_FULL, 5)
    mix, clean = synth.synth_utterances(8, 48000, 3, seed=93)
    x = torch.from_numpy(mix).cuda()
    src = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    lens = torch.full((8,), 48000, dtype=torch.int64, device="cuda")

    def run(hip):
        m = _model(FSN_FULL, sd, hip)
        pred, crm, s, xf = m.realtime_process(x, src, False, train=False)
        loss = m.compute_loss(src[:, 0], pred, xf, s, crm, lens)[0]
        loss.backward()
        out = float(loss.detach()), _flat(m)
        del m, pred, crm, s, xf, loss
        torch.cuda.empty_cache()
        return out

    l_t, g_t = run(False)
    l_h, g_h = run(True)
    l_h2, g_h2 = run(True)
    print(f"loss torch {l_t:.6f} HIP {l_h:.6f}; flat gradient rel {_rel(g_h, g_t):.2e}")
    assert abs(l_h - l_t) < 1e-4 * max(1.0, abs(l_t))
    assert _rel(g_h, g_t) < 3e-3
    assert l_h == l_h2 and torch.equal(g_h, g_h2)


def test_training_forward_matches_inference_and_continues_it():
    """pred of the training forward = FullSubNet.realtime_process(train=False) on the same weights (the same LSTM step kernels run,
    with the activations saved on the side), and the engine state it leaves continues a flag=True inference chunk exactly."""
    from speech_enhancement_mi_amd import synth
    from speech_enhancement_mi_amd.fullsubnet import FullSubNet
    sd = _sd(FSN_FULL, 7)
    mix, _ = synth.synth_utterances(2, 16000, 3, seed=95)
    x1, x2 = torch.from_numpy(mix[..., :9600].copy()).cuda(), torch.from_numpy(mix[..., 9600:].copy()).cuda()
    m = _model(FSN_FULL, sd, True)
    ref = FullSubNet(**FSN_FULL)
    ref.load_state_dict(sd)
    ref = ref.cuda()
    p_train = m.realtime_process(x1, flag=False, train=False)
    assert p_train.requires_grad
    with torch.no_grad():
        p_inf = ref.realtime_process(x1, flag=False, train=False)
        e = rel_rms(p_train.detach().cpu().numpy(), p_inf.cpu().numpy())
        print(f"training vs inference pred: rel rms {e:.2e}, max abs {float((p_train.detach() - p_inf).abs().max()):.2e}")
        assert e <= 1e-6
        c_train = m.realtime_process(x2, flag=True, train=False)
        c_inf = ref.realtime_process(x2, flag=True, train=False)
    assert torch.equal(c_train, c_inf)


def test_reference_training_loop_runs():
    """train_fullsubnet.py:137-145 unchanged on TrainableFullSubNet: GradScaler, accumulation 2, clip 5, Adam 3e-4
    (config.yaml:10,99-100); gradients stay finite and the loss falls on a fixed batch."""
    from speech_enhancement_mi_amd import synth
    sd = _sd(FSN_FULL, 9)
    model = _model(FSN_FULL, sd, True)
    mix, clean = synth.synth_utterances(4, 16000, 3, seed=97)
    mixture = torch.from_numpy(mix).cuda()
    source = torch.from_numpy(np.repeat(clean[:, None, :], 3, axis=1).copy()).cuda()
    length = torch.full((4,), 16000, dtype=torch.int64, device="cuda")
    optimizer = torch.optim.Adam(model.parameters(), lr=3e-4)
    scaler = torch.cuda.amp.GradScaler()
    gradient_accumulation, max_grad_norm = 2, 5
    losses = []
    for global_step in range(20):
        pred_source, pred_crm, sf, xf = model.realtime_process(mixture, source, torch.tensor([False] * 4), train=False)
        loss, logmse, sisnr = model.compute_loss(source[:, 0], pred_source, xf, sf, pred_crm, length)
        scaler.scale(loss / gradient_accumulation).backward()
        if (global_step + 1) % gradient_accumulation == 0:
            assert all(torch.isfinite(p.grad).all() for p in model.parameters())
            torch.nn.utils.clip_grad_norm_(filter(lambda p: p.requires_grad, model.parameters()), max_grad_norm)
            scaler.step(optimizer)
            scaler.update()
            optimizer.zero_grad()
        losses.append(float(loss.detach()))
    print("losses", [f"{v:.4f}" for v in losses])
    assert np.isfinite(losses).all()
    assert np.mean(losses[-4:]) < np.mean(losses[:4])
