"""Drop-in for the student architecture of the reference's distillation_crn.py (`TemporalCRN`, distillation_crn.py:
283-501; the distilled 0.81 M-parameter model is `TemporalCRN(num_channels=[16,32,64,64], hidden=128, ...)`,
distillation_crn.py:524-526).

Like the reference, `forward` returns `(y, [5 feature maps])` and `realtime_process` returns `(pred, [5 tensors of
[N*B, C_k, F_k, T]])` (distillation_crn.py:467-477): the pre-activation outputs of the last encoder convolution, of the
bottleneck's fc layer and of the first three transposed convolutions, which only the distillation *training* loss consumes.
The hot path fuses activations into the producing kernels, so the feature maps are produced by re-running those five kernels
without activation after every segment (engine taps "ft0".."ft4", written to device memory by `se_read_tap_dev`; they never cross the
host): set `return_features = False` for
inference (`predict_distillation.py:84` discards them) to get `(pred, None)` at full streaming speed."""
import ctypes as C

import torch
from torch import nn

from .crn import TemporalCRN as _Base
from .call_plan import call_plan, segment_geometry


class TemporalCRN(_Base):
    _VARIANT = 2
    return_features = True

    def _feature_shapes(self):
        c = self._cfg_args["num_channels"]
        L = len(c)
        F = [self.num_freqs]
        for _ in range(L):
            F.append((F[-1] - 1) // 2 + 1)
        return [(c[-1], F[L]), (c[-1], F[L])] + [(c[L - 2 - j], 2 * F[L - j] - 1) for j in range(L - 1)]

    def _features(self, eng, B):
        """The five taps of the segment just processed as DEVICE tensors [B, C*F, T] (se_read_tap_dev: the re-run kernels write
        device memory; nothing crosses the host)."""
        T = eng.T
        return [eng.read_tap_dev(f"ft{k}", B * ch * fr * T).view(B, ch * fr, T) for k, (ch, fr) in enumerate(self._feature_shapes())]

    def _shape_features(self, feats, B):
        return [f.reshape(f.shape[0], ch, fr, -1) for f, (ch, fr) in zip(feats, self._feature_shapes())]

    def forward(self, x):
        y = super().forward(x)
        if not self.return_features:
            return y, None
        feats = self._shape_features(self._features(self._eng, x.shape[0]), x.shape[0])
        return y, [f.to(x.device) for f in feats]

    def realtime_process(self, mixture, flag=False):
        if not self.return_features:
            return super().realtime_process(mixture, flag), None
        # segment by segment (utility.segmentation order, distillation_crn.py:455-471) so that the taps of every segment exist
        eng = self._engine_for(mixture)
        B, M, L = mixture.shape
        K = self.segment_length
        P = K // 2
        x = mixture.contiguous().float()
        if not flag:
            x = torch.nn.functional.pad(x, (P, 0))
            eng.reset(B)
        elif eng.batch != B:
            raise RuntimeError(f"flag=True with batch {B} but the carried state holds {eng.batch} streams")
        c = self._cfg_args
        g = segment_geometry(L, flag, K, int(round(c["sample_rate"] / 1000.0 * c["hop_length"])), c["n_fft"])
        Lp, gap, N = g["Lp"], g["gap"], g["N"]
        xp = torch.nn.functional.pad(x, (P, gap + P))
        segs, feats = [], None
        for n in range(N):
            segs.append(eng.step(xp[:, :, n * P:n * P + K].contiguous()))
            f = self._features(eng, B)
            feats = [[t] for t in f] if feats is None else [a + [t] for a, t in zip(feats, f)]
        y = torch.stack(segs, dim=1)  # [B, N, K]
        s1 = y[:, 0::2].reshape(B, -1)[:, P:]
        s2 = y[:, 1::2].reshape(B, -1)[:, :-P]
        out = ((s1 + s2) / 2)[:, :Lp]  # utility.over_add: average of the two streams, gap dropped
        if not flag:
            out = out[:, P:]
        ft = self._shape_features([torch.cat(f, dim=0) for f in feats], B)  # [N*B, C, F, T] (distillation_crn.py:473)
        return out, [f.to(mixture.device) for f in ft]

    def get_channel_num(self):  # distillation_crn.py:385-386
        c = self._cfg_args["num_channels"]
        return [c[-1], c[-1], c[2], c[1], c[0]]


EPS = 1e-8  # distillation_crn.py:11


def _flat_pair(t, s):
    """Teacher / student map -> [S][C][X] memory shared by both: the loss is per channel and elementwise, so the order inside (F, T)
    does not matter as long as the two agree.  The kernels' maps are transposed views of [S][C][T][F] tensors: undo the view."""
    for f in (lambda x: x, lambda x: x.transpose(-1, -2)):
        a, b = f(t), f(s)
        if a.is_contiguous() and b.is_contiguous():
            return a, b
    return t.contiguous(), s.contiguous()


class DistillLossFunction(torch.autograd.Function):
    """sum_i mean((BN(W_i s_i) - t'_i)^2 * mask_i) / n on the HIP kernels (se_distill_fwd / se_distill_bwd: one launch per pass for
    all maps, no float atomics).  forward(ctx, bns, training, n, s_0..s_{n-1}, t_0..t_{n-1}, (w, gamma, beta) x n); the BatchNorm
    running buffers of `bns` are updated on the device in training mode."""

    @staticmethod
    def _maps(ss, ts, ws, bns, grads=None):
        from .engine import SeDistillMap
        n = len(ss)
        arr = (SeDistillMap * n)()
        for i in range(n):
            m, bn = arr[i], bns[i]
            S, Cs = ss[i].shape[:2]
            Ct = ts[i].shape[1]
            m.s, m.t, m.w = ss[i].data_ptr(), ts[i].data_ptr(), ws[3 * i].data_ptr()
            m.gamma, m.beta = ws[3 * i + 1].data_ptr(), ws[3 * i + 2].data_ptr()
            m.running_mean, m.running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            m.num_batches_tracked = bn.num_batches_tracked.data_ptr()
            m.Cs, m.Ct, m.X = Cs, Ct, ss[i][0, 0].numel()
            if grads is not None:
                ds, dw, dg, db = grads[i]
                m.ds = None if ds is None else ds.data_ptr()
                m.dw, m.dgamma, m.dbeta = dw.data_ptr(), dg.data_ptr(), db.data_ptr()
        return arr

    @staticmethod
    def forward(ctx, bns, training, n, *args):
        from . import train_ops as K
        lib = K._lib()
        ss, ts, ws = list(args[:n]), list(args[n:2 * n]), list(args[2 * n:])
        K._need_gpu(*ss, *ts, *ws)
        S = ss[0].shape[0]
        for s, t in zip(ss, ts):
            if not (s.is_contiguous() and t.is_contiguous()) or s.shape[0] != S or t.shape[0] != S or s[0, 0].numel() != t[0, 0].numel():
                raise ValueError("distillation maps must be contiguous [S][C][X] with equal S and X for teacher and student")
        for i in range(n):
            Cs, Ct = ss[i].shape[1], ts[i].shape[1]
            if ws[3 * i].numel() != Ct * Cs or ws[3 * i + 1].numel() != Ct or ws[3 * i + 2].numel() != Ct or bns[i].running_mean.numel() != Ct:
                raise ValueError(f"connector {i} does not map {Cs} student to {Ct} teacher channels")
            if not all(w.is_contiguous() and w.dtype == torch.float32 for w in ws[3 * i:3 * i + 3]) or ss[i].dtype != torch.float32 or ts[i].dtype != torch.float32:
                raise ValueError("the distillation-loss kernels take contiguous fp32 tensors")
        arr = DistillLossFunction._maps(ss, ts, ws, bns)
        nb = lib.se_distill_ws_bytes(arr, n, S)
        K._chk(nb if nb < 0 else 0)
        wsp = torch.empty(nb, dtype=torch.uint8, device=ss[0].device)
        loss = torch.empty(1 + n, device=ss[0].device)
        with K._Timed("k_distill_fwd", 0.0):
            K._chk(lib.se_distill_fwd(arr, n, S, int(training), C.c_void_p(wsp.data_ptr()), C.c_void_p(loss.data_ptr()), K._st()))
        ctx.save_for_backward(*ss, *ts, *ws)
        ctx.n, ctx.bns, ctx.training, ctx.wsp, ctx.per_map = n, bns, training, wsp, loss[1:]
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gout):
        from . import train_ops as K
        lib = K._lib()
        n = ctx.n
        saved = ctx.saved_tensors
        ss, ts, ws = list(saved[:n]), list(saved[n:2 * n]), list(saved[2 * n:])
        grads = []
        for i in range(n):
            ds = torch.empty_like(ss[i]) if ctx.needs_input_grad[3 + i] else None
            grads.append((ds, torch.empty_like(ws[3 * i]), torch.empty_like(ws[3 * i + 1]), torch.empty_like(ws[3 * i + 2])))
        arr = DistillLossFunction._maps(ss, ts, ws, ctx.bns, grads)
        g = gout.reshape(1).contiguous().float()
        with K._Timed("k_distill_bwd", 0.0):
            K._chk(lib.se_distill_bwd(arr, n, ss[0].shape[0], int(ctx.training), C.c_void_p(ctx.wsp.data_ptr()), C.c_void_p(g.data_ptr()), K._st()))
        ctx.wsp = None
        out = [None, None, None] + [gr[0] for gr in grads] + [None] * n
        for gr in grads:
            out += list(gr[1:])
        return tuple(out)


class DistillationCRN(nn.Module):
    """Drop-in for the reference's DistillationCRN (distillation_crn.py:504-572), the model train_distillation.py trains: a frozen
    variant-2 teacher loaded from `path`, the 0.81 M-parameter student (num_channels [16, 32, 64, 64], hidden 128) whose parameters
    start as the teacher's where the shapes agree, and one 1x1 Conv2d + BatchNorm2d connector per feature map.  Same constructor and
    state_dict keys; forward(noisy, clean, length, flag) -> (loss, stoi, sisnr).

    The student parameters are copies of the teacher's (the reference shares the storage, but its trainer's .to(device) separates them
    again).  Like the reference, the model is never put in eval(): the BatchNorms use batch statistics and update their running
    buffers in every pass, no_grad passes included.

    Default: the torch restatement (CPU-runnable, the checker).  use_hip_kernels(True): the teacher's feature maps (no-grad forward
    from the torch parameters), the student's forward and backward (train_net.CRNFeatFunction) and the feature loss
    (DistillLossFunction) on the hand-written kernels; the teacher must then be frozen."""

    def __init__(self, *args, **kargs):
        super().__init__()
        from .training import TrainableStudentCRN
        model_path = kargs.pop("path", None)
        self.teacher = TrainableStudentCRN(*args, **kargs)
        if model_path is not None:
            self.teacher.load_state_dict(torch.load(model_path, map_location="cpu"))
            self.teacher.eval()
            for param in self.teacher.parameters():
                param.requires_grad = False
        kargs["num_channels"] = [16, 32, 64, 64]
        kargs["hidden"] = 128
        self.student = TrainableStudentCRN(*args, **kargs)
        with torch.no_grad():
            for pt, ps in zip(self.teacher.parameters(), self.student.parameters()):
                if ps.shape == pt.shape:
                    ps.copy_(pt)
        t_channels = self.teacher.get_channel_num()
        s_channels = self.student.get_channel_num()
        self.connectors = nn.ModuleList([self.build_feature_connector(t, s) for t, s in zip(t_channels, s_channels)])
        self._hip = False

    def build_feature_connector(self, t_channel, s_channel):
        C_ = [nn.Conv2d(s_channel, t_channel, kernel_size=1, stride=1, padding=0, bias=False), nn.BatchNorm2d(t_channel)]
        nn.init.kaiming_normal_(C_[0].weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(C_[1].weight, 1)
        nn.init.constant_(C_[1].bias, 0)
        return nn.Sequential(*C_)

    def use_hip_kernels(self, flag=True):
        self.teacher.use_hip_kernels(flag)
        self.student.use_hip_kernels(flag)
        self._hip = bool(flag)
        return self

    def get_margin(self, ft):
        mask = (ft < 0.0).float()
        masked_ft = ft * mask
        return masked_ft.sum(dim=(0, 2, 3), keepdim=True) / (mask.sum(dim=(0, 2, 3), keepdim=True) + EPS)

    def distillation_loss(self, ft, fs):
        """distillation_crn.py:555-566."""
        if self._hip:
            return self._distillation_loss_hip(ft, fs)
        loss = 0.0
        for i in range(len(ft)):
            t, s = ft[i], fs[i]
            margin = self.get_margin(t)
            t = torch.max(t, margin)
            s = self.connectors[i](s)
            mask = 1.0 - ((s <= t) & (t <= 0.0)).float()
            loss += torch.mean((s - t) ** 2 * mask)
        return loss / len(ft)

    def _distillation_loss_hip(self, ft, fs):
        bns = [c[1] for c in self.connectors]
        training = bns[0].training
        for bn in bns:
            if bn.training != training or bn.momentum != 0.1 or bn.eps != 1e-5 or not (bn.affine and bn.track_running_stats):
                raise ValueError("the distillation-loss kernels implement BatchNorm2d(momentum=0.1, eps=1e-5, affine, running statistics)")
        pairs = [_flat_pair(t.detach(), s) for t, s in zip(ft, fs)]
        ts = [t.reshape(t.shape[0], t.shape[1], -1) for t, _ in pairs]
        ss = [s.reshape(s.shape[0], s.shape[1], -1) for _, s in pairs]
        params = []
        for c in self.connectors:
            params += [c[0].weight, c[1].weight, c[1].bias]
        return DistillLossFunction.apply(bns, training, len(ss), *ss, *ts, *params)

    def forward(self, noisy, clean, length, flag):
        """flag and length per utterance: a batch of chunk chains (datagen.ChunkChainBatch) - teacher and student see utterance b up to
        length[b] only and continue their own row b where flag[b] holds; a batch of full-length utterances with one flag is the plain call."""
        B, Lmax = noisy.shape[0], noisy.shape[-1]
        st = self.student
        plan = call_plan(flag, length, B, Lmax, st.segment_length, st._hop, st._nfft)
        if plan.uniform:
            return self._forward(noisy, clean, length, plan.flag, {})
        return self._forward(noisy, clean, length, plan.flags, dict(lengths=plan.lengths))

    def _forward(self, noisy, clean, length, flag, kw):
        if self._hip:
            if any(p.requires_grad for p in self.teacher.parameters()):
                raise RuntimeError("the HIP distillation path needs a frozen teacher (DistillationCRN(..., path=checkpoint)); "
                                   "a trainable teacher runs on the torch path only")
            with torch.no_grad():
                _, ft = self.teacher.realtime_process_train(noisy, flag, features=True, **kw)
        else:
            _, ft = self.teacher.realtime_process_train(noisy, flag, features=True, **kw)
        pred, fs = self.student.realtime_process_train(noisy, flag, features=True, **kw)
        loss, stoi, sisnr = self.student.compute_loss(clean, pred, length)
        loss = loss + self.distillation_loss(ft, fs)
        return loss, stoi, sisnr
