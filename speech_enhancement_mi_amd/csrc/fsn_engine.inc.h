// fsn_engine.inc.h - FullSubNet engine behind the fsn_* C ABI (include/se_engine.h); included at the end of se_engine.hip
// (one translation unit, so the kernels in the shared headers are defined once).
// Reference: FullSubNet.forward / realtime_process(train=False), fullsubnet.py:769-824, 903-961.

struct fsn_engine : EngineHost {
    fsn_config c{};
    int T = 0, F = 0, M = 0, K = 0, N = 0, Kp = 0, SI = 0, NL = 0;
    bool weights_ready = false;
    SigChain sig;  // STFT / iSTFT tables and plan (sig_chain.h)
    struct Model {
        int in = 0, inp = 0, H = 0, out = 0;
        DevBuf Wp[4], bias[4];      // per layer: bf16x3 planes of [W_ih | W_hh] (K padded to 32s), b_ih + b_hh
        DevBuf fcw, fcw_x, fcb;
        DevBuf h[4][2], c[4];       // state
        int hcur[4]{};
        DevBuf whh_t[4], wih_t[4];  // training backward (fp32): W_hh^T [H][4H], W_ih^T [in][4H] (layers >= 1)
        DevBuf wcol, fcw_t;         // sub-band: column SI - 1 of W_ih_l0 [4H]; full-band: fc weight^T [H][Fp] (zero padded)
    } fb, sb;
    int B = 0;
    DevBuf spec, maskspec, mag, fb_seq, fb_out, sbin, mask, part_fb, part_sb, mean_fb, mean_sb, denom_fb, denom_sb, yseg;
    int nslot_fb = 0, nslot_sb = 0;
    // CumLayerNorm step counters (fullsubnet.py:192-198): one int per stream and norm, on the device (k_fsn_runmean); 0 = no mean yet
    DevBuf step_fb, step_sb;
    // fsn_realtime_process_chains.  Bact > 0: the stages run for the prefix of Bact streams (grids, LSTM / GEMM / STFT rows); B stays every
    // allocation and time stride.  plan_dev: the device copy of the call's ChainPlan vectors (chain_plan.h).  carry_*: the rows of the
    // streams that ended before the longest one (state_rows.hip.h, fsn_state_rows_of).
    int Bact = 0;
    DevBuf plan_dev, carry_h[2][4], carry_c[2][4], carry_mean[2], carry_step[2];
    // realtime_process: the full-band model of window n + 1 runs on `side` while the sub-band model of window n runs on the caller's stream
    // (the full-band recurrence is 42 launches of 32 workgroups per window, 11 % of the serial time, latency-bound: profiles/r03_fsn_*)
    hipStream_t side = nullptr;
    hipEvent_t ev_ready[2]{}, ev_consumed[2]{}, ev_done[2]{}, ev_fork = nullptr;
    // ... and inside stage B the sub-band model's layer 1 runs one time step behind layer 0 on `side2`: both launches are 4.7 rounds of
    // one-workgroup-per-CU tiles, the second fills the first one's last round
    hipStream_t side2 = nullptr;
    std::vector<hipEvent_t> ev_l0, ev_l1;  // per time step: layer 0 / layer 1 (+ its output layer) done
    // fsn_train_fwd: where the stages save the activations of window `tr_n` (fsn_train.inc.h); null in inference
    const struct FsnTrainLayout *tr = nullptr;
    float *tr_ws = nullptr;
    int tr_n = 0;
    bool train_ready = false;  // the fp32 transposed weights of the backward are uploaded
    int pipeline = 1;     // SE_FSN_PIPELINE=0: one stream, stage after stage (read at fsn_create)
    int lstm_big = 1;     // SE_FSN_BIG=0: keep the 128 x 128 step tiles where the 256-row x 64-unit tile would be picked (read at fsn_create)
};

// Float offsets into the workspace of fsn_train_fwd / fsn_train_bwd (include/se_engine.h).  Model index 0 = full band (S = base[N]
// rows per step: N*B, or the packed sum of bact(n) of a chains call), 1 = sub band (S * F rows).  Every saved tensor is [T][S][.]: step t
// of ALL N windows is one contiguous slab, window n's rows at base[n] (*F) inside it, so one backward launch per step covers every
// window (the state is detached at each seam).
struct FsnTrainLayout {
    int B = 0, N = 0;
    long S[2]{};
    std::vector<long> base;                        // full-band row of window n's first stream, n = 0 .. N (base[N] = S[0])
    size_t hdr = 0;                                // chains: the plan's staging vector (8 B floats), then the packed row table (S[0] ints)
    size_t gates[2][4]{}, cs[2][4]{}, hs[2][4]{};  // gates i, f, g, o [T][S][4H]; c, h [T + 1][S][H], slot 0 = the state entering the window
    size_t xs[2]{};                                // layer-0 inputs: full band [T][S][Kp] (normalised |X|), sub band [T][S][SI]
    size_t fbo = 0;                                // full-band output after the ReLU [T][S][F]
    size_t denom = 0;                              // sub-band CumLayerNorm denominators of every window [N][B]
    size_t dg = 0, dcf = 0, dx = 0, dm = 0, dpre = 0, wsum = 0, csum = 0, tmp = 0;  // backward scratch
    size_t total = 0;
};

namespace {

int fsn_prepare(fsn_engine *e) {
    if (e->weights_ready) return 0;
    struct { fsn_engine::Model *m; const char *name; } models[2] = {{&e->fb, "fb_model"}, {&e->sb, "sb_model"}};
    for (auto &mm : models) {
        fsn_engine::Model &m = *mm.m;
        const int H = m.H, Hp = (H + 31) & ~31;
        for (int l = 0; l < e->NL; l++) {
            const std::string p = std::string(mm.name) + ".sequence_model.", s = std::to_string(l);
            const int in = l == 0 ? m.in : H, inp = l == 0 ? m.inp : Hp;
            auto *wih = param(e, p + "weight_ih_l" + s, 4 * (size_t)H * in);
            auto *whh = param(e, p + "weight_hh_l" + s, 4 * (size_t)H * H);
            auto *bih = param(e, p + "bias_ih_l" + s, 4 * (size_t)H);
            auto *bhh = param(e, p + "bias_hh_l" + s, 4 * (size_t)H);
            if (!wih || !whh || !bih || !bhh) return SE_ERR_PARAM_MISSING;
            const int Kt = inp + Hp;
            std::vector<float> cat((size_t)4 * H * Kt, 0.0f), bias(4 * (size_t)H);
            for (int r = 0; r < 4 * H; r++) {
                for (int k = 0; k < in; k++) cat[(size_t)r * Kt + k] = (*wih)[(size_t)r * in + k];
                for (int k = 0; k < H; k++) cat[(size_t)r * Kt + inp + k] = (*whh)[(size_t)r * H + k];
                bias[r] = (*bih)[r] + (*bhh)[r];
            }
            int rc;
            if ((rc = upload_planes(e, m.Wp[l], cat, 0)) || (rc = dev_upload(e, m.bias[l], bias))) return rc;
        }
        auto *fw = param(e, std::string(mm.name) + ".fc_output_layer.weight", (size_t)m.out * H);
        auto *fbv = param(e, std::string(mm.name) + ".fc_output_layer.bias", m.out);
        if (!fw || !fbv) return SE_ERR_PARAM_MISSING;
        int rc;
        if ((rc = dev_upload(e, m.fcw, *fw)) || (rc = upload_planes(e, m.fcw_x, *fw, 0)) || (rc = dev_upload(e, m.fcb, *fbv))) return rc;
    }
    e->weights_ready = true;
    return 0;
}

// training forward, before window e->tr_n's LSTM: its layer-0 input (element (r, t, k) at x[r*sR + t*sT + k], W columns) -> xs[mi] and
// each layer's entering state (h, c) -> slot 0 of hs / cs
int fsn_train_save_window(fsn_engine *e, int mi, const float *x, long sR, long sT, int W, int R, hipStream_t st) {
    const FsnTrainLayout &L = *e->tr;
    fsn_engine::Model &m = mi ? e->sb : e->fb;
    const long S = L.S[mi], r0 = L.base[e->tr_n] * (mi ? e->F : 1);
    hipLaunchKernelGGL(k_fsn_save_rows, dim3(2048), dim3(256), 0, st, x, sR, sT, W, R, e->T, e->tr_ws + L.xs[mi] + r0 * W, S * W);
    HIPCHECK(e, hipGetLastError());
    for (int l = 0; l < e->NL; l++) {
        const size_t n = (size_t)R * m.H;
        HIPCHECK(e, hipMemcpyAsync(e->tr_ws + L.hs[mi][l] + r0 * m.H, m.h[l][m.hcur[l]].p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIPCHECK(e, hipMemcpyAsync(e->tr_ws + L.cs[mi][l] + r0 * m.H, m.c[l].p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

// t >= 0 and e->tr set (fsn_train_fwd): step t of window e->tr_n, saving gates, c_t and h_t into the training workspace
int fsn_lstm_step(fsn_engine *e, fsn_engine::Model &m, int l, const float *x, long ldx, int K1, int K1p, int R, float *hseq, long ldseq, hipStream_t st,
                  int t = -1) {
    const int hc = m.hcur[l];
    LstmStepArgs a{x, ldx, K1, K1p, m.h[l][hc].p, reinterpret_cast<const __bf16 *>(m.Wp[l].p), m.bias[l].p, m.c[l].p, m.h[l][hc ^ 1].p, hseq, ldseq, R, m.H};
    if (e->tr && t >= 0) {  // all training steps take the 128 x 128 tile (at R = B*F = 1 608 per window the step is latency-bound anyway)
        const FsnTrainLayout &L = *e->tr;
        const int mi = &m == &e->sb ? 1 : 0;
        const long S = L.S[mi], r0 = L.base[e->tr_n] * (mi ? e->F : 1), H = m.H;
        a.gsave = e->tr_ws + L.gates[mi][l] + ((long)t * S + r0) * 4 * H;
        a.csave = e->tr_ws + L.cs[mi][l] + ((long)(t + 1) * S + r0) * H;
        a.hsave = e->tr_ws + L.hs[mi][l] + ((long)(t + 1) * S + r0) * H;
        const dim3 grid((m.H + 31) / 32, (R + kGemmBM - 1) / kGemmBM);
        if (e->c.precision == 2) hipLaunchKernelGGL((k_lstm_step_x6<2, true>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_lstm_step_x6<3, true>), grid, dim3(256), 0, st, a);
        m.hcur[l] = hc ^ 1;
        return 0;
    }
#ifdef SE_LSTM_STAMPS
    static unsigned long long *stamps = nullptr;
    static int nlaunch = 0;
    if (!stamps) { (void)hipMalloc(&stamps, 64); (void)hipMemset(stamps, 0, 64); }
    a.stamps = stamps;
    if (R >= 8192 && ++nlaunch % 997 == 0) {
        (void)hipStreamSynchronize(st);
        unsigned long long h[7];
        (void)hipMemcpy(h, stamps, sizeof h, hipMemcpyDeviceToHost);
        if (e->lstm_big == 1)
            fprintf(stderr, "[stamps big] before layer %d: nck %llu per-chunk cycles: barrier1 %.0f store+wait %.0f barrier2 %.0f gate0 %.0f dma+issue %.0f rest %.0f\n", l, h[6],
                    (double)h[0] / h[6], (double)h[1] / h[6], (double)h[2] / h[6], (double)h[3] / h[6], (double)h[4] / h[6], (double)h[5] / h[6]);
        else
            fprintf(stderr, "[stamps] before layer %d: nck %llu per-chunk cycles: barrier1 %.0f vmwait %.0f stage %.0f barrier2 %.0f issue+mfma %.0f\n", l, h[5],
                    (double)h[0] / h[5], (double)h[1] / h[5], (double)h[2] / h[5], (double)h[3] / h[5], (double)h[4] / h[5]);
    }
#endif
    // big tile (256 rows x 64 units) where it fills the chip: the sub-band model at B >= 32 streams
    // (the carried batch picks the route, not the active prefix of a chains call: one kernel for a stream from its first window to its last)
    const long Rroute = (long)e->B * (&m == &e->sb ? e->F : 1);
    if (e->lstm_big == 1 && m.H % kLbU == 0 && Rroute >= 32 * kLbM) {
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_lstm_step_big<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_lstm_step_big<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            attr = true;
        }
        const dim3 gb(m.H / kLbU, (R + kLbM - 1) / kLbM);
        const int PL = e->c.precision == 2 ? 2 : 3;
        const size_t lds = (size_t)(PL == 2 ? 4 : 3) * PL * kLbPlane * sizeof(__bf16);  // bf16x3: both operands double-buffered
        if (PL == 2) hipLaunchKernelGGL((k_lstm_step_big<2>), gb, dim3(512), lds, st, a);
        else hipLaunchKernelGGL((k_lstm_step_big<3>), gb, dim3(512), lds, st, a);
        m.hcur[l] = hc ^ 1;
        return 0;
    }
    const dim3 grid((m.H + 31) / 32, (R + kGemmBM - 1) / kGemmBM);
    if (e->c.precision == 2) hipLaunchKernelGGL((k_lstm_step_x6<2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_lstm_step_x6<3>), grid, dim3(256), 0, st, a);
    m.hcur[l] = hc ^ 1;
    return 0;
}

// forward on device.  Spectrum given by (re, im) pointers + strides in float units for (b, m, t, f).
// Stage A of a window: |X|, its CumLayerNorm, the full-band LSTM and its output layer -> e->mag, e->fb_out (read by stage B's unfold only)
int fsn_stage_fb(fsn_engine *e, const float *re, const float *im, long sB, long sM, long sT, long sF, hipStream_t st) {
    const int B = e->Bact > 0 ? e->Bact : e->B, T = e->T, F = e->F, M = e->M, Kp = e->Kp;
    {  // |X| + CumLayerNorm of the full-band input (fullsubnet.py:782-788)
        FsnMagArgs a{re, im, sB, sM, sT, sF, e->mag.p, e->part_fb.p, M, T, F, Kp};
        hipLaunchKernelGGL(k_fsn_mag, dim3(e->nslot_fb, B), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_fsn_runmean, dim3((B + 255) / 256), dim3(256), 0, st, e->part_fb.p, e->nslot_fb, (double)M * T * F, e->mean_fb.p,
                           e->denom_fb.p, B, reinterpret_cast<int *>(e->step_fb.p));
        hipLaunchKernelGGL(k_fsn_scale, dim3(16, B), dim3(256), 0, st, e->mag.p, (long)T * Kp, e->denom_fb.p);
        HIPCHECK(e, hipGetLastError());
    }
    if (e->tr) {  // training forward: the layer-0 input and the state entering the window
        int rc = fsn_train_save_window(e, 0, e->mag.p, (long)T * Kp, Kp, Kp, B, st);
        if (rc) return rc;
    }
    for (int t = 0; t < T; t++) {  // full-band LSTM (2 layers interleaved per step), fullsubnet.py:789
        for (int l = 0; l < e->NL; l++) {
            const bool last = l + 1 == e->NL;
            if (l == 0) fsn_lstm_step(e, e->fb, 0, e->mag.p + (long)t * Kp, (long)T * Kp, Kp, Kp, B, last ? e->fb_seq.p + (long)t * e->fb.H : nullptr, (long)T * e->fb.H, st, t);
            else fsn_lstm_step(e, e->fb, l, e->fb.h[l - 1][e->fb.hcur[l - 1]].p, e->fb.H, e->fb.H, (e->fb.H + 31) & ~31, B,
                               last ? e->fb_seq.p + (long)t * e->fb.H : nullptr, (long)T * e->fb.H, st, t);
        }
    }
    HIPCHECK(e, hipGetLastError());
    {  // fc_output_layer + ReLU (fullsubnet.py:288-290): [B*T, H] -> [B*T, F]
        GemmX6Args g{e->fb_seq.p, reinterpret_cast<const __bf16 *>(e->fb.fcw_x.p), e->fb.fcb.p, e->fb_out.p, B * T, F, e->fb.H, (long)e->fb.H, (long)F, 1};
        hipLaunchKernelGGL(k_gemm_x<3>, dim3((F + kGemmBN - 1) / kGemmBN, (B * T + kGemmBM - 1) / kGemmBM), dim3(256), 0, st, g);
    }
    HIPCHECK(e, hipGetLastError());
    if (e->tr) {  // fb_out [B*T][F] -> [T][S][F] (its sign is the ReLU's derivative)
        const FsnTrainLayout &L = *e->tr;
        hipLaunchKernelGGL(k_fsn_save_rows, dim3(1024), dim3(256), 0, st, e->fb_out.p, (long)T * F, (long)F, F, B, T,
                           e->tr_ws + L.fbo + L.base[e->tr_n] * F, L.S[0] * F);
        HIPCHECK(e, hipGetLastError());
    }
    return 0;
}

// Stage B: sub-band input, its CumLayerNorm, the sub-band LSTM over B*F rows, mask.  `consumed` (optional) is recorded once e->mag / e->fb_out
// have been read, i.e. when the next window's stage A may overwrite them.
int fsn_stage_sb(fsn_engine *e, const float *re, const float *im, long sB, long sT, long sF, float *crm_out, cf2 *spec_out,
                 long oB, long oT, long oF, hipStream_t st, hipEvent_t consumed) {
    const int B = e->Bact > 0 ? e->Bact : e->B, T = e->T, F = e->F, Kp = e->Kp, SI = e->SI;
    const int R = B * F;
    const long Rall = (long)e->B * F;  // sbin's time stride: the carried batch, whatever prefix of it this window runs for
    {  // sub-band input + its CumLayerNorm (fullsubnet.py:796-802)
        FsnUnfoldArgs a{e->mag.p, e->fb_out.p, e->sbin.p, e->part_sb.p, e->B, T, F, Kp, e->c.sb_neighbors, SI};
        hipLaunchKernelGGL(k_fsn_unfold, dim3(e->nslot_sb, B), dim3(256), 0, st, a);
        if (consumed) HIPCHECK(e, hipEventRecord(consumed, st));
        hipLaunchKernelGGL(k_fsn_runmean, dim3((B + 255) / 256), dim3(256), 0, st, e->part_sb.p, e->nslot_sb, (double)F * SI * T, e->mean_sb.p,
                           e->denom_sb.p, B, reinterpret_cast<int *>(e->step_sb.p));
        hipLaunchKernelGGL(k_fsn_scale_sb, dim3(2048), dim3(256), 0, st, e->sbin.p, e->B, T, F, SI, e->denom_sb.p, B);
        HIPCHECK(e, hipGetLastError());
    }
    if (e->tr) {  // training forward: the normalised sub-band input, this window's denominators, the state entering the window
        HIPCHECK(e, hipMemcpyAsync(e->tr_ws + e->tr->denom + e->tr->base[e->tr_n], e->denom_sb.p, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, st));
        int rc = fsn_train_save_window(e, 1, e->sbin.p, SI, Rall * SI, SI, R, st);
        if (rc) return rc;
    }
    // two layers (the reference configuration) on two streams: layer 0 of step t + 1 next to layer 1 of step t.  h of layer 0 ping-pongs
    // between two buffers: step t + 2 of layer 0 overwrites what layer 1 of step t reads, hence ev_l1[t].
    const bool wave = consumed != nullptr && e->side2 && e->NL == 2 && (int)e->ev_l0.size() >= T;
    for (int t = 0; t < T; t++) {  // sub-band LSTM over B*F rows + Linear(H -> 2)  (fullsubnet.py:812-814)
        for (int l = 0; l < e->NL; l++) {
            hipStream_t sl = wave && l == 1 ? e->side2 : st;
            if (wave && l == 0 && t >= 2) HIPCHECK(e, hipStreamWaitEvent(st, e->ev_l1[t - 2], 0));
            if (wave && l == 1) HIPCHECK(e, hipStreamWaitEvent(sl, e->ev_l0[t], 0));
            if (l == 0) fsn_lstm_step(e, e->sb, 0, e->sbin.p + (long)t * Rall * SI, SI, SI, (SI + 31) & ~31, R, nullptr, 0, sl, t);
            else fsn_lstm_step(e, e->sb, l, e->sb.h[l - 1][e->sb.hcur[l - 1]].p, e->sb.H, e->sb.H, (e->sb.H + 31) & ~31, R, nullptr, 0, sl, t);
            if (wave && l == 0) HIPCHECK(e, hipEventRecord(e->ev_l0[t], st));
        }
        const int ll = e->NL - 1;
        hipStream_t so = wave ? e->side2 : st;
        hipLaunchKernelGGL(k_fsn_sbfc, dim3(2048), dim3(256), 0, so, e->sb.h[ll][e->sb.hcur[ll]].p, e->sb.fcw.p, e->sb.fcb.p, e->mask.p, R, e->sb.H, T, t);
        if (wave) HIPCHECK(e, hipEventRecord(e->ev_l1[t], so));
    }
    if (wave) HIPCHECK(e, hipStreamWaitEvent(st, e->ev_l1[T - 1], 0));  // join: the mask needs every step's output
    HIPCHECK(e, hipGetLastError());
    {
        FsnMaskArgs a{e->mask.p, spec_out ? re : nullptr, spec_out ? im : nullptr, sB, sT, sF, spec_out, oB, oT, oF, crm_out, T, F};
        launch_k_fsn_mask(dim3((T * F + 255) / 256, B), st, a);
        HIPCHECK(e, hipGetLastError());
    }
    return 0;
}

int fsn_forward_dev(fsn_engine *e, const float *re, const float *im, long sB, long sM, long sT, long sF, float *crm_out, cf2 *spec_out,
                    long oB, long oT, long oF, hipStream_t st) {
    int rc;
    if ((rc = fsn_stage_fb(e, re, im, sB, sM, sT, sF, st))) return rc;
    return fsn_stage_sb(e, re, im, sB, sT, sF, crm_out, spec_out, oB, oT, oF, st, nullptr);
}

int fsn_reset_on(fsn_engine *e, int batch, hipStream_t st) {
    if (!e || batch <= 0) return fail(e, SE_ERR_ARG, "batch must be positive");
    HIPCHECK(e, hipSetDevice(e->device));
    int rc = fsn_prepare(e);
    if (rc) return rc;
    const int B = batch, T = e->T, F = e->F, M = e->M, R = B * F;
    e->B = B;
    e->nslot_fb = 8;
    e->nslot_sb = 32;
    // spec holds two windows: stage A of window n + 1 transforms while stage B of window n still masks its spectrum
    if ((rc = dev_alloc(e, e->spec, (size_t)2 * B * M * T * F * 2)) || (rc = dev_alloc(e, e->maskspec, (size_t)B * T * F * 2)) ||
        (rc = dev_alloc(e, e->mag, (size_t)B * T * e->Kp)) || (rc = dev_alloc(e, e->fb_seq, (size_t)B * T * e->fb.H)) ||
        (rc = dev_alloc(e, e->fb_out, (size_t)B * T * F)) || (rc = dev_alloc(e, e->sbin, (size_t)T * R * e->SI)) ||
        (rc = dev_alloc(e, e->mask, (size_t)R * 2 * T)) || (rc = dev_alloc(e, e->part_fb, (size_t)B * e->nslot_fb)) ||
        (rc = dev_alloc(e, e->part_sb, (size_t)B * e->nslot_sb)) || (rc = dev_alloc(e, e->mean_fb, B)) || (rc = dev_alloc(e, e->mean_sb, B)) ||
        (rc = dev_alloc(e, e->denom_fb, B)) || (rc = dev_alloc(e, e->denom_sb, B)) || (rc = dev_alloc(e, e->step_fb, B)) || (rc = dev_alloc(e, e->step_sb, B)))
        return rc;
    HIPCHECK(e, hipMemsetAsync(e->mag.p, 0, (size_t)B * T * e->Kp * sizeof(float), st));  // padding columns must be zero
    for (int l = 0; l < e->NL; l++) {
        for (int p = 0; p < 2; p++) {
            if ((rc = dev_alloc(e, e->fb.h[l][p], (size_t)B * e->fb.H)) || (rc = dev_alloc(e, e->sb.h[l][p], (size_t)R * e->sb.H))) return rc;
            HIPCHECK(e, hipMemsetAsync(e->fb.h[l][p].p, 0, (size_t)B * e->fb.H * sizeof(float), st));
            HIPCHECK(e, hipMemsetAsync(e->sb.h[l][p].p, 0, (size_t)R * e->sb.H * sizeof(float), st));
        }
        if ((rc = dev_alloc(e, e->fb.c[l], (size_t)B * e->fb.H)) || (rc = dev_alloc(e, e->sb.c[l], (size_t)R * e->sb.H))) return rc;
        HIPCHECK(e, hipMemsetAsync(e->fb.c[l].p, 0, (size_t)B * e->fb.H * sizeof(float), st));
        HIPCHECK(e, hipMemsetAsync(e->sb.c[l].p, 0, (size_t)R * e->sb.H * sizeof(float), st));
        e->fb.hcur[l] = e->sb.hcur[l] = 0;
    }
    HIPCHECK(e, hipMemsetAsync(e->step_fb.p, 0, (size_t)B * sizeof(int), st));  // both norms: no mean yet (CumLayerNorm.reset)
    HIPCHECK(e, hipMemsetAsync(e->step_sb.p, 0, (size_t)B * sizeof(int), st));
    e->Bact = 0;
    return 0;
}

}  // namespace

// ---- WHERE a stream's carried state lives: f(live tensor, carry buffer, words per stream row) for every state tensor of model mi ----
// mi 0 = the full-band set (h, c of every layer, mean_fb, step_fb), 1 = the sub-band set (the same of the sub-band model; its rows are
// the stream's F sub-band rows).  h lives in the half hcur[l] points at NOW.  Stops at the first f that returns non-zero.
template <class Fn>
static int fsn_state_rows_of(fsn_engine *e, int mi, Fn &&f) {
    static_assert(2 * 4 + 2 <= kStateRowsMax, "state row table too small");
    fsn_engine::Model &m = mi ? e->sb : e->fb;
    const long per = (long)(mi ? e->F : 1) * m.H;
    int rc;
    for (int l = 0; l < e->NL; l++)
        if ((rc = f(m.h[l][m.hcur[l]].p, e->carry_h[mi][l], per)) || (rc = f(m.c[l].p, e->carry_c[mi][l], per))) return rc;
    if ((rc = f(mi ? e->mean_sb.p : e->mean_fb.p, e->carry_mean[mi], 1L))) return rc;
    return f(mi ? e->step_sb.p : e->step_fb.p, e->carry_step[mi], 1L);
}

extern "C" {

const char *fsn_last_error(const fsn_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int fsn_create(const fsn_config *cfg, int device, fsn_engine **out) {
    if (!cfg || !out) return fail(nullptr, SE_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->fb_neighbors != 0 || cfg->look_ahead != 0) return fail(nullptr, SE_ERR_ARG, "only fb_num_neighbors = 0, look_ahead = 0 (config.yaml:154-157) are supported");
    if (cfg->num_layers < 1 || cfg->num_layers > 4) return fail(nullptr, SE_ERR_ARG, "num_layers %d out of range", cfg->num_layers);
    if (cfg->fb_hidden % 8 || cfg->sb_hidden % 8 || cfg->fb_hidden <= 0 || cfg->sb_hidden <= 0) return fail(nullptr, SE_ERR_ARG, "hidden sizes must be positive multiples of 8");
    if ((2 * cfg->sb_neighbors + 2) % 4) return fail(nullptr, SE_ERR_ARG, "sub-band input width 2*sb_num_neighbors+2 must be a multiple of 4");
    if (cfg->precision != 0 && cfg->precision != 2) return fail(nullptr, SE_ERR_ARG, "fsn precision %d unknown (0 fp32-accurate, 2 bf16x3)", cfg->precision);
    if (cfg->n_fft % 2 || cfg->num_freqs != cfg->n_fft / 2 + 1) return fail(nullptr, SE_ERR_ARG, "num_freqs must be n_fft/2+1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SE_ERR_HIP, "no HIP device available: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, SE_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    fsn_engine *e = new fsn_engine();
    std::string why;
    if (int rc = sig_chain_create(e->sig, cfg->n_fft, cfg->win, cfg->hop, cfg->segment_length, device, why)) { delete e; return fail(nullptr, rc, "%s", why.c_str()); }
    // the floor the engine has always had: inherited from the CRN geometry it used to be checked against, not FullSubNet's own
    if (e->sig.T <= 16) {
        sig_chain_destroy(e->sig);
        delete e;
        return fail(nullptr, SE_ERR_ARG, "segment_length %d at hop %d gives %d frames per segment: more than 16 frames are required", cfg->segment_length, cfg->hop,
                    1 + cfg->segment_length / cfg->hop);
    }
    e->c = *cfg; e->device = device;
    e->T = e->sig.T; e->F = cfg->num_freqs; e->M = cfg->num_mics; e->K = cfg->segment_length; e->N = cfg->n_fft; e->NL = cfg->num_layers;
    e->Kp = (cfg->num_freqs * cfg->num_mics + 31) & ~31;
    e->SI = 2 * cfg->sb_neighbors + 2;
    e->fb.in = cfg->num_freqs * cfg->num_mics; e->fb.inp = e->Kp; e->fb.H = cfg->fb_hidden; e->fb.out = cfg->num_freqs;
    e->sb.in = e->SI; e->sb.inp = (e->SI + 31) & ~31; e->sb.H = cfg->sb_hidden; e->sb.out = 2;
    if (const char *s = getenv("SE_FSN_BIG")) e->lstm_big = atoi(s);
    if (const char *s = getenv("SE_FSN_PIPELINE")) e->pipeline = atoi(s);
    if (e->pipeline) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        bool ok = hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, hi) == hipSuccess;  // the short full-band launches go first when a CU frees up
        ok = ok && hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2 && ok; i++)
            ok = hipEventCreateWithFlags(&e->ev_ready[i], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e->ev_consumed[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&e->ev_done[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&e->side2, hipStreamNonBlocking) == hipSuccess;
        e->ev_l0.assign(e->T, nullptr); e->ev_l1.assign(e->T, nullptr);
        for (int t = 0; t < e->T && ok; t++)
            ok = hipEventCreateWithFlags(&e->ev_l0[t], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&e->ev_l1[t], hipEventDisableTiming) == hipSuccess;
        if (!ok) { fsn_destroy(e); return fail(nullptr, SE_ERR_HIP, "fsn_create: side stream / events: %s", hipGetErrorString(hipGetLastError())); }
    }
    *out = e;
    return SE_OK;
}

void fsn_destroy(fsn_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    for (fsn_engine::Model *m : {&e->fb, &e->sb}) {
        for (int l = 0; l < 4; l++) {
            dev_free(m->Wp[l]); dev_free(m->bias[l]); dev_free(m->h[l][0]); dev_free(m->h[l][1]); dev_free(m->c[l]);
            dev_free(m->whh_t[l]); dev_free(m->wih_t[l]);
        }
        dev_free(m->fcw); dev_free(m->fcw_x); dev_free(m->fcb); dev_free(m->wcol); dev_free(m->fcw_t);
    }
    for (DevBuf *b : {&e->spec, &e->maskspec, &e->mag, &e->fb_seq, &e->fb_out, &e->sbin, &e->mask, &e->part_fb, &e->part_sb, &e->mean_fb,
                      &e->mean_sb, &e->denom_fb, &e->denom_sb, &e->yseg, &e->step_fb, &e->step_sb, &e->plan_dev, &e->carry_mean[0], &e->carry_mean[1],
                      &e->carry_step[0], &e->carry_step[1]})
        dev_free(*b);
    for (int mi = 0; mi < 2; mi++)
        for (int l = 0; l < 4; l++) { dev_free(e->carry_h[mi][l]); dev_free(e->carry_c[mi][l]); }
    if (e->side) (void)hipStreamDestroy(e->side);
    if (e->side2) (void)hipStreamDestroy(e->side2);
    for (hipEvent_t ev : e->ev_l0) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->ev_l1) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : {e->ev_fork, e->ev_ready[0], e->ev_ready[1], e->ev_consumed[0], e->ev_consumed[1], e->ev_done[0], e->ev_done[1]})
        if (ev) (void)hipEventDestroy(ev);
    sig_chain_destroy(e->sig);
    delete e;
}

int fsn_load_param(fsn_engine *e, const char *key, const float *host_data, const int64_t *shape, int ndim) {
    if (!e || !key || !host_data) return fail(e, SE_ERR_ARG, "null argument");
    const std::string k(key);
    bool ok = false;
    for (const char *mname : {"fb_model.", "sb_model."}) {
        if (k.rfind(mname, 0) != 0) continue;
        const std::string rest = k.substr(9);
        int l = -1, n = 0;
        char what[32];
        if (sscanf(rest.c_str(), "sequence_model.%31[a-z_]%d%n", what, &l, &n) == 2)
            ok = l >= 0 && l < e->NL && (size_t)n == rest.size() &&
                 (!strcmp(what, "weight_ih_l") || !strcmp(what, "weight_hh_l") || !strcmp(what, "bias_ih_l") || !strcmp(what, "bias_hh_l"));
        else ok = rest == "fc_output_layer.weight" || rest == "fc_output_layer.bias";
    }
    if (!ok) return fail(e, SE_ERR_KEY, "unknown parameter key %s", key);
    e->weights_ready = false;
    e->train_ready = false;
    return store_param(e, k, host_data, shape, ndim);
}

int fsn_reset(fsn_engine *e, int batch) {
    int rc = fsn_reset_on(e, batch, nullptr);
    if (rc) return rc;
    HIPCHECK(e, hipDeviceSynchronize());
    return SE_OK;
}

// FullSubNet.forward: x [B, 2M, F, T] (re x M then im x M) -> crm [B, 2, F, T]
int fsn_forward(fsn_engine *e, const float *x, float *crm, void *stream) {
    if (!e || !x || !crm) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "fsn_forward before fsn_reset");
    HIPCHECK(e, hipSetDevice(e->device));
    int rc = fsn_prepare(e);
    if (rc) return rc;
    const long F = e->F, T = e->T, M = e->M;
    return fsn_forward_dev(e, x, x + M * F * T, 2 * M * F * T, F * T, 1, T, crm, nullptr, 0, 0, 0, static_cast<hipStream_t>(stream));
}

// the rows of the streams a ChainPlan names: which bit mi = model mi, dir 0 save, 1 restore, 2 zero.  One launch per model.
static int fsn_chain_rows(fsn_engine *e, unsigned which, int dir, StreamRange r, hipStream_t st) {
    if (r.count <= 0) return 0;
    for (int mi = 0; mi < 2; mi++) {
        if (!(which & (1u << mi))) continue;
        StateRowList rows;
        fsn_state_rows_of(e, mi, [&](float *live, DevBuf &carry, long words) { rows.add(live, carry.p, words); return 0; });
        rows.launch(st, dir, r.streams, r.count);
        HIPCHECK(e, hipGetLastError());
    }
    return 0;
}

static int fsn_alloc_carry(fsn_engine *e) {
    int rc = 0;
    for (int mi = 0; mi < 2 && !rc; mi++)
        rc = fsn_state_rows_of(e, mi, [&](float *, DevBuf &carry, long words) { return dev_alloc(e, carry, (size_t)e->B * words); });
    return rc;
}

// The windows of one realtime_process call on state that is ready: Nseg half-overlapping windows, window n of a stream starting at
// n*K/2 + off0 (uniform) or n*K/2 + ch->off0[b] (chains), STFT -> stage A -> stage B -> iSTFT, then the overlap average with `skip` (or
// ch->skip[b]) stripped.  ch: the chains call's ChainPlan (chain_plan.h), null for the uniform call.
static int fsn_run_windows(fsn_engine *e, const float *mixture, int batch, long length, long Nseg, long off0, long skip, float *out, hipStream_t st,
                           const ChainPlan *ch) {
    int rc;
    const long K = e->K, P = K / 2;
    if ((rc = dev_alloc(e, e->yseg, (size_t)batch * Nseg * K))) return rc;
    const long F = e->F, T = e->T, M = e->M;
    cf2 *spec = reinterpret_cast<cf2 *>(e->spec.p);
    cf2 *ms = reinterpret_cast<cf2 *>(e->maskspec.p);
    const size_t spec_floats = (size_t)batch * M * T * F * 2;
    const bool piped = e->pipeline && e->side && Nseg > 1;
    hipStream_t sa = piped ? e->side : st;
    if (piped) {  // the side stream starts after whatever the caller's stream holds (reset, the previous call's tail)
        HIPCHECK(e, hipEventRecord(e->ev_fork, st));
        HIPCHECK(e, hipStreamWaitEvent(sa, e->ev_fork, 0));
    }
    struct Scope {  // a failing call leaves the engine usable: nothing of the plan outlives the call
        fsn_engine *e;
        ~Scope() { e->Bact = 0; }
    } scope{e};
    const SigRows rows = ch ? SigRows{ch->len, ch->off0} : SigRows{};
    for (long n = 0; n < Nseg; n++) {
        const long off = n * P + (ch ? 0 : off0);
        const int slot = piped ? (int)(n & 1) : 0;
        const float *sp = e->spec.p + slot * spec_floats;
        const int bact = ch ? ch->bact(n) : batch;
        const StreamRange last = ch ? ch->ending(n) : StreamRange{nullptr, 0};  // the streams whose last window this is
        if (ch) e->Bact = bact;
        if (piped) {
            if (n >= 2) HIPCHECK(e, hipStreamWaitEvent(sa, e->ev_done[slot], 0));          // window n - 2 has masked spectrum[slot]
            if (n >= 1) HIPCHECK(e, hipStreamWaitEvent(sa, e->ev_consumed[slot ^ 1], 0));  // window n - 1 has unfolded mag / fb_out
        }
        HIPCHECK(e, sig_stft(e->sig, mixture, (long)M * length, length, (int)M, off, length, rows, bact * (int)M, spec + slot * (spec_floats / 2), T * F, F, 1, sa));
        if ((rc = fsn_stage_fb(e, sp, sp + 1, 2 * M * T * F, 2 * T * F, 2 * F, 2, sa))) return rc;
        // the full-band stage of window n + 1 runs ahead on `side`: the full-band rows of the streams that end here are kept now, on `side`
        if ((rc = fsn_chain_rows(e, 1u, 0, last, sa))) return rc;
        if (piped) {
            HIPCHECK(e, hipEventRecord(e->ev_ready[slot], sa));
            HIPCHECK(e, hipStreamWaitEvent(st, e->ev_ready[slot], 0));
        }
        if ((rc = fsn_stage_sb(e, sp, sp + 1, 2 * M * T * F, 2 * F, 2, nullptr, ms, T * F, F, 1, st, piped ? e->ev_consumed[slot] : nullptr))) return rc;
        if ((rc = fsn_chain_rows(e, 2u, 0, last, st))) return rc;  // stage B has joined `side2`
        HIPCHECK(e, sig_istft(e->sig, ms, T * F, F, 1, bact, e->yseg.p + n * K, Nseg * K, st));
        if (piped) HIPCHECK(e, hipEventRecord(e->ev_done[slot], st));
    }
    // the streams that ended before the longest one get their own state back (the last stage B waited for everything on `side`)
    if (ch && (rc = fsn_chain_rows(e, 3u, 1, ch->ended_early(), st))) return rc;
    launch_k_overlap_avg(dim3((unsigned)((length + 255) / 256), batch), st, e->yseg.p, out, (int)Nseg, (int)K, (long)length, skip, rows.len,
                         ch ? ch->skip : nullptr);
    HIPCHECK(e, hipGetLastError());
    return SE_OK;
}

// FullSubNet.realtime_process(mixture, source, flag, train=False)[0]: mixture [B, M, L] -> [B, L]
int fsn_realtime_process(fsn_engine *e, const float *mixture, int batch, int64_t length, int flag, float *out, void *stream) {
    if (!e || !mixture || !out || batch <= 0 || length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (!flag) { if ((rc = fsn_reset_on(e, batch, st))) return rc; }
    else {
        if (e->B != batch) return fail(e, SE_ERR_STATE, "flag=True with batch %d but the carried state holds %d streams", batch, e->B);
        HIPCHECK(e, hipSetDevice(e->device));
        if ((rc = fsn_prepare(e))) return rc;
    }
    const ChunkGeometry g = chunk_geometry(e->K, length, flag);
    return fsn_run_windows(e, mixture, batch, length, g.nseg, g.off0, g.skip, out, st, nullptr);
}

// A batch of chunk chains (include/se_engine.h): reset or prepare, plan (chain_plan.h), upload, zero the flag-0 rows and counters, run
int fsn_realtime_process_chains(fsn_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host,
                                float *out, void *stream) {
    if (!e || !mixture || !out || !lengths_host || !flags_host || batch <= 0 || max_length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    ChainPlan plan;
    std::string err;
    int uniform_flag = 0;
    int rc = plan_chains(plan, e->K, batch, max_length, lengths_host, flags_host, e->B, &uniform_flag, err);
    if (rc == kPlanUniform) return fsn_realtime_process(e, mixture, batch, max_length, uniform_flag, out, stream);
    if (rc) return fail(e, rc, "%s", err.c_str());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!plan.continues()) rc = fsn_reset_on(e, batch, st);
    else {
        HIPCHECK(e, hipSetDevice(e->device));
        rc = fsn_prepare(e);
    }
    if (rc) return rc;
    if ((rc = fsn_alloc_carry(e)) || (rc = upload_plan(e, e->plan_dev, plan, st))) return rc;
    // a reset among continuing streams: zero those streams' rows and counters (fsn_reset_stream for any number of streams in two launches)
    if (plan.continues() && (rc = fsn_chain_rows(e, 3u, 2, plan.reset_streams(), st))) return rc;
    return fsn_run_windows(e, mixture, batch, max_length, plan.N, 0, 0, out, st, &plan);
}

// reset_state + both CumLayerNorm.reset() (fullsubnet.py:826-832, 203-205) for ONE stream of the carried batch
int fsn_reset_stream(fsn_engine *e, int stream_index, void *stream) {
    if (!e) return SE_ERR_ARG;
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "fsn_reset_stream before fsn_reset");
    if (stream_index < 0 || stream_index >= e->B) return fail(e, SE_ERR_ARG, "stream index %d outside the batch of %d", stream_index, e->B);
    HIPCHECK(e, hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = 0;
    for (int mi = 0; mi < 2 && !rc; mi++)
        rc = fsn_state_rows_of(e, mi, [&](float *live, DevBuf &, long words) {
            HIPCHECK(e, hipMemsetAsync(live + words * stream_index, 0, (size_t)words * sizeof(float), st));
            return 0;
        });
    return rc;
}

// the tensor behind a state name: fh / fc / sh / sc -> per layer (l < NL) a device pointer and its length; mean_* / step_* -> one vector
static int fsn_state_of(fsn_engine *e, const char *name, float *ptr[4], size_t *per_layer, int *layers, bool *is_step) {
    const size_t B = (size_t)e->B;
    *is_step = false;
    if (!strcmp(name, "fh") || !strcmp(name, "fc") || !strcmp(name, "sh") || !strcmp(name, "sc")) {
        fsn_engine::Model &m = name[0] == 's' ? e->sb : e->fb;
        for (int l = 0; l < e->NL; l++) ptr[l] = name[1] == 'h' ? m.h[l][m.hcur[l]].p : m.c[l].p;
        *per_layer = B * (name[0] == 's' ? e->F : 1) * m.H;  // sub band: row b*F + f, the reference's [num_freqs * batch] order (fullsubnet.py:810-811, 829)
        *layers = e->NL;
        return 0;
    }
    *layers = 1;
    *per_layer = B;
    if (!strcmp(name, "mean_fb")) ptr[0] = e->mean_fb.p;
    else if (!strcmp(name, "mean_sb")) ptr[0] = e->mean_sb.p;
    else if (!strcmp(name, "step_fb")) { ptr[0] = e->step_fb.p; *is_step = true; }
    else if (!strcmp(name, "step_sb")) { ptr[0] = e->step_sb.p; *is_step = true; }
    else return fail(e, SE_ERR_KEY, "unknown state %s", name);
    return 0;
}

int fsn_export_state(fsn_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream) {
    if (!e || !name || !host_out) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no state: call fsn_reset first");
    float *ptr[4];
    size_t per = 0;
    int layers = 0, rc;
    bool is_step = false;
    if ((rc = fsn_state_of(e, name, ptr, &per, &layers, &is_step))) return rc;
    const size_t n = per * layers;
    if (count) *count = (int64_t)n;
    if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int l = 0; l < layers; l++) HIPCHECK(e, hipMemcpy(host_out + (size_t)l * per, ptr[l], per * sizeof(float), hipMemcpyDeviceToHost));
    if (is_step)  // the counters are ints on the device, small integers held exactly as floats outside
        for (size_t i = 0; i < n; i++) { int v; memcpy(&v, host_out + i, sizeof v); host_out[i] = (float)v; }
    return SE_OK;
}

int fsn_import_state(fsn_engine *e, const char *name, const float *host_in, int64_t count, void *stream) {
    if (!e || !name || !host_in) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no state: call fsn_reset first");
    float *ptr[4];
    size_t per = 0;
    int layers = 0, rc;
    bool is_step = false;
    if ((rc = fsn_state_of(e, name, ptr, &per, &layers, &is_step))) return rc;
    if (count != (int64_t)(per * layers)) return fail(e, SE_ERR_SHAPE, "state %s needs %zu floats", name, per * layers);
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    if (is_step) {
        std::vector<int> v(per);
        for (size_t i = 0; i < per; i++) {
            if (!(host_in[i] >= 0.0f && host_in[i] <= 80.0f) || host_in[i] != (float)(int)host_in[i])
                return fail(e, SE_ERR_ARG, "state %s: %g is not a step count in 0 .. 80", name, (double)host_in[i]);
            v[i] = (int)host_in[i];
        }
        HIPCHECK(e, hipMemcpy(ptr[0], v.data(), per * sizeof(int), hipMemcpyHostToDevice));
        return SE_OK;
    }
    for (int l = 0; l < layers; l++) HIPCHECK(e, hipMemcpy(ptr[l], host_in + (size_t)l * per, per * sizeof(float), hipMemcpyHostToDevice));
    return SE_OK;
}

int fsn_read_tap(fsn_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream) {
    if (!e || !name || !host_out) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no forward has run");
    const float *src = nullptr;
    size_t n = 0;
    if (!strcmp(name, "fb_out")) { src = e->fb_out.p; n = (size_t)e->B * e->T * e->F; }          // [B*T][F]
    else if (!strcmp(name, "mean_fb")) { src = e->mean_fb.p; n = e->B; }
    else if (!strcmp(name, "mean_sb")) { src = e->mean_sb.p; n = e->B; }
    else return fail(e, SE_ERR_KEY, "unknown tap %s", name);
    if (count) *count = (int64_t)n;
    if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
    HIPCHECK(e, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    HIPCHECK(e, hipMemcpy(host_out, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return SE_OK;
}

double fsn_flops_per_frame(const fsn_engine *e) {
    if (!e) return 0;
    double mac = 0;
    const fsn_engine::Model *ms[2] = {&e->fb, &e->sb};
    const double rows[2] = {1.0, (double)e->F};
    for (int i = 0; i < 2; i++) {
        const fsn_engine::Model &m = *ms[i];
        for (int l = 0; l < e->NL; l++) mac += rows[i] * e->T * 4.0 * m.H * ((l == 0 ? m.in : m.H) + m.H);
        mac += rows[i] * e->T * (double)m.out * m.H;
    }
    return 2.0 * mac;
}

}  // extern "C"
