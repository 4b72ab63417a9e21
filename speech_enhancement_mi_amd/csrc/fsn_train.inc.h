// fsn_train.inc.h - FullSubNet training behind fsn_train_ws_bytes / fsn_train_fwd / fsn_train_bwd (include/se_engine.h); included at
// the end of se_engine.hip after fsn_engine.inc.h and train_ops.inc.h.
// Reference: train_fullsubnet.py:137-145 (autograd over realtime_process(train=False), fullsubnet.py:903-961, one forward per window,
// fullsubnet.py:769-824).  The LSTM state (fh, sh) is detached after every window (fullsubnet.py:819-820), so the BPTT of window n
// starts from window n - 1's state as a constant, and the N windows' sequences are independent in the backward: each BPTT step is ONE
// launch over S = N x rows sequences (k_lstm_bwd_step).  Both CumLayerNorms divide by a detached running mean (fullsubnet.py:200):
// their gradient is 1 / (mean + EPS) of the window.  Weight gradients: se_train_gemm_tn_det + se_train_colsum (fixed order, no
// float atomics); input gradients: se_train_gemm (fp32-exact MFMA).

namespace {

// the offsets for base[N] full-band rows per step; hdr_floats = the chains header (0: none, and the total of before)
void fsn_train_layout(const fsn_engine *e, int B, int N, std::vector<long> base, size_t hdr_floats, FsnTrainLayout &L) {
    const long T = e->T, F = e->F, Hf = e->fb.H, Hs = e->sb.H, Kp = e->Kp, SI = e->SI, Fp = (F + 7) & ~7L;
    L = FsnTrainLayout{};
    L.B = B; L.N = N;
    L.S[0] = base[N];
    L.S[1] = base[N] * F;
    L.base = std::move(base);
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 63) & ~(size_t)63; return o; };
    const long Hm[2] = {Hf, Hs};
    for (int mi = 0; mi < 2; mi++)
        for (int l = 0; l < e->NL; l++) {
            const long S = L.S[mi], H = Hm[mi];
            L.gates[mi][l] = take((size_t)T * S * 4 * H);
            L.cs[mi][l] = take((size_t)(T + 1) * S * H);
            L.hs[mi][l] = take((size_t)(T + 1) * S * H);
        }
    L.xs[0] = take((size_t)T * L.S[0] * Kp);
    L.xs[1] = take((size_t)T * L.S[1] * SI);
    L.fbo = take((size_t)T * L.S[0] * F);
    L.denom = take((size_t)L.S[0]);
    const size_t sh = std::max((size_t)L.S[0] * Hf, (size_t)L.S[1] * Hs);
    L.dg = take((size_t)T * std::max((size_t)L.S[0] * 4 * Hf, (size_t)L.S[1] * 4 * Hs));
    L.dcf = take(sh);
    L.dx = take((size_t)T * sh);
    L.dm = take((size_t)T * L.S[1] * 2);
    L.dpre = take((size_t)T * L.S[0] * Fp);
    const size_t nw = std::max({(size_t)4 * Hf * Kp, (size_t)4 * Hf * Hf, (size_t)4 * Hs * SI, (size_t)4 * Hs * Hs, (size_t)Fp * Hf, (size_t)2 * Hs});
    L.wsum = take(64 * nw);
    L.csum = take((size_t)((T * L.S[1] + 63) / 64 + (T * L.S[0] + 63) / 64) * std::max({4 * Hf, 4 * Hs, Fp}));
    L.tmp = take(nw);
    L.hdr = take(hdr_floats);
    L.total = off;
}

// one flag, one length: every stream runs every window, window n's rows at n*B
int fsn_train_plan(const fsn_engine *e, int B, int N, FsnTrainLayout &L) {
    std::vector<long> base((size_t)N + 1);
    for (int n = 0; n <= N; n++) base[n] = (long)n * B;
    fsn_train_layout(e, B, N, std::move(base), 0, L);
    return 0;
}

// A batch of chunk chains (fsn_train_*_chains): the call's ChainPlan (chain_plan.h: geometry, validation and error texts are the
// planner's) and the layout it implies.  PACKED when the plan is compact (window counts non-increasing): window n runs for the prefix of
// bact(n) streams and saves its activations at rows base[n] = sum_{m<n} bact(m), so S[0] = sum_n bact(n) and the dead windows cost no
// workspace, no BPTT rows and no weight-gradient rows; rowmap[packed row] = n*B + b is what k_fsn_gather_dm reads the dense dcrm
// through.  Otherwise (a carried batch keeps its slots) the dense layout: every stream runs every window.
// The backward rebuilds this plan from the same host arguments (the geometry is a few integers per stream); the device copies - the
// plan's staging vector and the row table - are uploaded once, by the forward, into the header region of ws, where the backward finds
// the row table again.
struct FsnTrainChains {
    ChainPlan plan;
    FsnTrainLayout L;
    std::vector<int> rowmap;  // empty: dense
    bool packed() const { return !rowmap.empty(); }
};

// kPlanUniform (*nseg, *uniform_flag set: the plain call serves it), kPlanFilled, or an error (e->err set).  carried: the streams whose
// state the engine holds (the backward passes `batch`: its forward has been accepted, whatever ran on the engine since)
int fsn_train_plan_chains(fsn_engine *e, int carried, int batch, int64_t max_length, const int64_t *lengths, const uint8_t *flags, FsnTrainChains &c,
                          int *nseg, int *uniform_flag) {
    std::string err;
    const int rc = plan_chains(c.plan, e->K, batch, max_length, lengths, flags, carried, uniform_flag, err);
    if (rc == kPlanUniform) { *nseg = (int)chunk_geometry(e->K, max_length, *uniform_flag).nseg; return rc; }
    if (rc) return fail(e, rc, "%s", err.c_str());
    const ChainPlan &p = c.plan;
    std::vector<long> base((size_t)p.N + 1, 0);
    for (int n = 0; n < p.N; n++) base[n + 1] = base[n] + p.bact(n);
    c.rowmap.clear();
    if (p.compact) {
        c.rowmap.resize((size_t)base[p.N]);
        for (int n = 0; n < p.N; n++)
            for (int b = 0; b < p.bact(n); b++) c.rowmap[(size_t)base[n] + b] = n * batch + b;
    }
    *nseg = p.N;
    fsn_train_layout(e, batch, p.N, std::move(base), p.staging_floats() + c.rowmap.size(), c.L);
    return kPlanFilled;
}

int fsn_prepare_train(fsn_engine *e) {
    int rc = fsn_prepare(e);
    if (rc) return rc;
    if (e->train_ready) return 0;
    struct { fsn_engine::Model *m; const char *name; } models[2] = {{&e->fb, "fb_model"}, {&e->sb, "sb_model"}};
    for (auto &mm : models) {
        fsn_engine::Model &m = *mm.m;
        const int H = m.H;
        for (int l = 0; l < e->NL; l++) {
            const std::string p = std::string(mm.name) + ".sequence_model.", s = std::to_string(l);
            const int in = l == 0 ? m.in : H;
            auto *wih = param(e, p + "weight_ih_l" + s, 4 * (size_t)H * in);
            auto *whh = param(e, p + "weight_hh_l" + s, 4 * (size_t)H * H);
            if (!wih || !whh) return SE_ERR_PARAM_MISSING;
            std::vector<float> t((size_t)H * 4 * H);
            for (int r = 0; r < 4 * H; r++)
                for (int k = 0; k < H; k++) t[(size_t)k * 4 * H + r] = (*whh)[(size_t)r * H + k];
            if ((rc = dev_upload(e, m.whh_t[l], t))) return rc;
            if (l > 0) {
                for (int r = 0; r < 4 * H; r++)
                    for (int k = 0; k < H; k++) t[(size_t)k * 4 * H + r] = (*wih)[(size_t)r * H + k];
                if ((rc = dev_upload(e, m.wih_t[l], t))) return rc;
            } else if (&m == &e->sb) {  // the sub-band input's last column is fb_out (fb_num_neighbors = 0): the only one with a gradient
                std::vector<float> col(4 * (size_t)H);
                for (int r = 0; r < 4 * H; r++) col[r] = (*wih)[(size_t)r * in + in - 1];
                if ((rc = dev_upload(e, m.wcol, col))) return rc;
            }
        }
    }
    const int F = e->F, Fp = (F + 7) & ~7, Hf = e->fb.H;
    auto *fw = param(e, "fb_model.fc_output_layer.weight", (size_t)F * Hf);
    if (!fw) return SE_ERR_PARAM_MISSING;
    std::vector<float> t((size_t)Hf * Fp, 0.0f);
    for (int f = 0; f < F; f++)
        for (int k = 0; k < Hf; k++) t[(size_t)k * Fp + f] = (*fw)[(size_t)f * Hf + k];
    if ((rc = dev_upload(e, e->fb.fcw_t, t))) return rc;
    e->train_ready = true;
    return 0;
}

// The windows of one training forward on state that is ready, on ONE stream in window order (norm update, full band, unfold, sub band:
// the engine's own per-window order).  ch: the chains call's ChainPlan, null for the uniform call.  With ch, window n runs for the prefix
// of ch->bact(n) streams (all of them unless the plan is compact); the state rows of the streams whose last window this is are saved
// before window n + 1 touches them, and every stream that ended before the longest one gets its own rows back after the last window.
int fsn_train_windows(fsn_engine *e, const float *spec, int batch, const FsnTrainLayout &L, float *ws, float *crm_out, hipStream_t st, const ChainPlan *ch) {
    struct Scope {  // a failing call leaves the engine usable
        fsn_engine *e;
        ~Scope() { e->tr = nullptr; e->tr_ws = nullptr; e->Bact = 0; }
    } scope{e};
    const long M = e->M, T = e->T, F = e->F;
    e->tr = &L;
    e->tr_ws = ws;
    int rc = 0;
    for (int n = 0; n < L.N; n++) {
        e->tr_n = n;
        if (ch) e->Bact = ch->bact(n);
        const float *sp = spec + (size_t)n * batch * M * T * F * 2;
        float *crm = crm_out + (size_t)n * batch * 2 * F * T;
        if ((rc = fsn_stage_fb(e, sp, sp + 1, 2 * M * T * F, 2 * T * F, 2 * F, 2, st))) return rc;
        if ((rc = fsn_stage_sb(e, sp, sp + 1, 2 * M * T * F, 2 * F, 2, crm, nullptr, 0, 0, 0, st, nullptr))) return rc;
        if (!ch) continue;
        if ((rc = fsn_chain_rows(e, 3u, 0, ch->ending(n), st))) return rc;
        // Dense route: a stream past its own last window still runs.  It reads an all-zero spectrum, the rows it dirties are restored
        // below, and its crm is cleared here, so its dcrm is an exact zero (the mask backward multiplies by the zero spectrum).  Every
        // backward stage maps an exact zero to an exact zero, and the CumLayerNorm denominators of such windows are
        // mean(sqrt(EPS)) + EPS > 0, so nothing non-finite can arise from them.
        if (!ch->compact)
            for (int b = 0; b < batch; b++)
                if (ch->nseg[b] <= n) HIPCHECK(e, hipMemsetAsync(crm + (size_t)b * 2 * F * T, 0, (size_t)2 * F * T * sizeof(float), st));
    }
    if (ch && (rc = fsn_chain_rows(e, 3u, 1, ch->ended_early(), st))) return rc;
    return 0;
}

int tchk(fsn_engine *e, int rc) { return rc ? fail(e, rc, "%s", se_train_last_error()) : 0; }

// all T steps of layer l of model mi, last step first; dG of every step stays in L.dg for the weight gradients
int fsn_bptt(fsn_engine *e, const FsnTrainLayout &L, float *ws, int mi, int l, const float *dout, const float *dm, const float *wfc, hipStream_t st) {
    const fsn_engine::Model &m = mi ? e->sb : e->fb;
    const long S = L.S[mi], H = m.H, T = e->T;
    const dim3 grid((unsigned)((H + kLbwBN - 1) / kLbwBN), (unsigned)((S + kLbwBM - 1) / kLbwBM));
    for (long t = T - 1; t >= 0; t--) {
        LstmBwdArgs a{};
        a.dgn = t + 1 < T ? ws + L.dg + (t + 1) * S * 4 * H : nullptr;
        a.whh_t = m.whh_t[l].p;
        a.dout = dout ? dout + t * S * H : nullptr;
        a.dm = dm ? dm + t * S * 2 : nullptr;
        a.wfc = wfc;
        a.gates = ws + L.gates[mi][l] + t * S * 4 * H;
        a.cprev = ws + L.cs[mi][l] + t * S * H;
        a.ccur = ws + L.cs[mi][l] + (t + 1) * S * H;
        a.dcf = ws + L.dcf;
        a.dg = ws + L.dg + t * S * 4 * H;
        a.S = (int)S; a.H = (int)H;
        hipLaunchKernelGGL(k_lstm_bwd_step, grid, dim3(256), 0, st, a);
    }
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// out[rows][cols] (dense) = the leading block of sum_r A[r][:Na]^T X[r][:Nb]
int fsn_wgrad(fsn_engine *e, const FsnTrainLayout &L, float *ws, const float *A, const float *X, long R, int Na, int Nb, float *out, int rows, int cols,
              hipStream_t st) {
    int ns = 0, rc;
    if ((rc = tchk(e, se_train_gemm_tn_det(A, X, ws + L.wsum, &ns, R, Na, Nb, st)))) return rc;
    if ((rc = tchk(e, se_train_colsum(ws + L.wsum, ws + L.tmp, Na * Nb, nullptr, nullptr, 0, nullptr, nullptr, 0, ns, 0, st)))) return rc;
    HIPCHECK(e, hipMemcpy2DAsync(out, (size_t)cols * sizeof(float), ws + L.tmp, (size_t)Nb * sizeof(float), (size_t)cols * sizeof(float), rows,
                             hipMemcpyDeviceToDevice, st));
    return 0;
}

// out1 (and out2, may be null) [n] = column sums of x [R][ld], first n columns
int fsn_bgrad(fsn_engine *e, const FsnTrainLayout &L, float *ws, const float *x, long R, int ld, int n, float *out1, float *out2, hipStream_t st) {
    int rc;
    if ((rc = tchk(e, se_train_colsum_tall(x, R, ld, ws + L.csum, ws + L.tmp, 0, st)))) return rc;
    for (float *o : {out1, out2})
        if (o) HIPCHECK(e, hipMemcpyAsync(o, ws + L.tmp, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}

int fsn_train_bwd_rows(fsn_engine *e, const float *dcrm, const FsnTrainLayout &L, const int *rowmap, void *wsp, float *const *grads, int ngrads, void *stream);

}  // namespace

extern "C" {

int64_t fsn_train_ws_bytes(fsn_engine *e, int batch, int nseg) {
    if (!e || batch <= 0 || nseg <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    FsnTrainLayout L;
    fsn_train_plan(e, batch, nseg, L);
    return (int64_t)(L.total * sizeof(float));
}

int fsn_train_fwd(fsn_engine *e, const float *spec, int batch, int nseg, int flag, void *ws, float *crm_out, void *stream) {
    if (!e || !spec || !ws || !crm_out || batch <= 0 || nseg <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHECK(e, hipSetDevice(e->device));
    int rc;
    if (!flag) { if ((rc = fsn_reset_on(e, batch, st))) return rc; }
    else if (e->B != batch) return fail(e, SE_ERR_STATE, "flag=True with batch %d but the carried state holds %d streams", batch, e->B);
    if ((rc = fsn_prepare(e))) return rc;
    FsnTrainLayout L;
    fsn_train_plan(e, batch, nseg, L);
    return fsn_train_windows(e, spec, batch, L, static_cast<float *>(ws), crm_out, st, nullptr);
}

int64_t fsn_train_ws_bytes_chains(fsn_engine *e, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host) {
    if (!e || !lengths_host || !flags_host || batch <= 0 || max_length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    FsnTrainChains c;
    int nseg = 0, uflag = 0;
    const int rc = fsn_train_plan_chains(e, e->B, batch, max_length, lengths_host, flags_host, c, &nseg, &uflag);
    if (rc == kPlanUniform) return fsn_train_ws_bytes(e, batch, nseg);
    if (rc) return rc;
    return (int64_t)(c.L.total * sizeof(float));
}

// reset or prepare, plan, upload the header, zero the flag-0 rows and counters among continuing streams, run the windows
int fsn_train_fwd_chains(fsn_engine *e, const float *spec, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host, void *ws,
                         float *crm_out, void *stream) {
    if (!e || !spec || !ws || !crm_out || !lengths_host || !flags_host || batch <= 0 || max_length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    FsnTrainChains c;
    int nseg = 0, uflag = 0;
    int rc = fsn_train_plan_chains(e, e->B, batch, max_length, lengths_host, flags_host, c, &nseg, &uflag);
    if (rc == kPlanUniform) return fsn_train_fwd(e, spec, batch, nseg, uflag, ws, crm_out, stream);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ChainPlan &plan = c.plan;
    if (!plan.continues()) rc = fsn_reset_on(e, batch, st);
    else {
        HIPCHECK(e, hipSetDevice(e->device));
        rc = fsn_prepare(e);
    }
    if (rc || (rc = fsn_alloc_carry(e))) return rc;
    float *wsf = static_cast<float *>(ws);
    std::vector<int32_t> hdr(plan.staging_floats() + c.rowmap.size());
    memcpy(hdr.data(), plan.staging.data(), plan.staging.size() * sizeof(int64_t));
    if (c.packed()) memcpy(hdr.data() + plan.staging_floats(), c.rowmap.data(), c.rowmap.size() * sizeof(int));
    HIPCHECK(e, hipMemcpyAsync(wsf + c.L.hdr, hdr.data(), hdr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(e, hipStreamSynchronize(st));  // the header and the host arrays live for the call only
    plan.carve(wsf + c.L.hdr);
    if (plan.continues() && (rc = fsn_chain_rows(e, 3u, 2, plan.reset_streams(), st))) return rc;
    // dead windows (n >= the stream's own count) hold exact zeros: the packed route never writes them, the dense route clears them
    HIPCHECK(e, hipMemsetAsync(crm_out, 0, (size_t)plan.N * batch * 2 * e->F * e->T * sizeof(float), st));
    return fsn_train_windows(e, spec, batch, c.L, wsf, crm_out, st, &plan);
}

int fsn_train_bwd(fsn_engine *e, const float *dcrm, int batch, int nseg, void *wsp, float *const *grads, int ngrads, void *stream) {
    if (!e || !dcrm || !wsp || !grads || batch <= 0 || nseg <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    FsnTrainLayout L;
    fsn_train_plan(e, batch, nseg, L);
    return fsn_train_bwd_rows(e, dcrm, L, nullptr, wsp, grads, ngrads, stream);
}

int fsn_train_bwd_chains(fsn_engine *e, const float *dcrm, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host, void *wsp,
                         float *const *grads, int ngrads, void *stream) {
    if (!e || !dcrm || !wsp || !grads || !lengths_host || !flags_host || batch <= 0 || max_length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    FsnTrainChains c;
    int nseg = 0, uflag = 0;
    const int rc = fsn_train_plan_chains(e, batch, batch, max_length, lengths_host, flags_host, c, &nseg, &uflag);
    if (rc == kPlanUniform) return fsn_train_bwd(e, dcrm, batch, nseg, wsp, grads, ngrads, stream);
    if (rc) return rc;
    // the row table the forward left in the header of ws, behind the plan's staging vector
    const int *rowmap = c.packed() ? reinterpret_cast<const int *>(static_cast<const float *>(wsp) + c.L.hdr + c.plan.staging_floats()) : nullptr;
    return fsn_train_bwd_rows(e, dcrm, c.L, rowmap, wsp, grads, ngrads, stream);
}

}  // extern "C"

namespace {

// the backward over the L.S[0] rows of the layout (dense or packed: the kernels see a flat S); rowmap: device, packed row -> n*B + b
int fsn_train_bwd_rows(fsn_engine *e, const float *dcrm, const FsnTrainLayout &L, const int *rowmap, void *wsp, float *const *grads, int ngrads, void *stream) {
    const int NL = e->NL;
    if (ngrads != 2 * (4 * NL + 2)) return fail(e, SE_ERR_ARG, "expected %d gradient pointers, got %d", 2 * (4 * NL + 2), ngrads);
    for (int i = 0; i < ngrads; i++)
        if (!grads[i]) return fail(e, SE_ERR_ARG, "gradient pointer %d is null", i);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHECK(e, hipSetDevice(e->device));
    int rc;
    if ((rc = fsn_prepare_train(e))) return rc;
    float *ws = static_cast<float *>(wsp);
    const int T = e->T, F = e->F, Fp = (F + 7) & ~7, Hf = e->fb.H, Hs = e->sb.H;
    const long S0 = L.S[0], S1 = L.S[1], R0 = (long)T * S0, R1 = (long)T * S1;
    float *const *gfb = grads, *const *gsb = grads + 4 * NL + 2;  // per model: (W_ih, W_hh, b_ih, b_hh) x layers, fc weight, fc bias

    // sub band: Linear(H -> 2) (no activation) over the last layer, then the layers top down
    hipLaunchKernelGGL(k_fsn_gather_dm, dim3(2048), dim3(256), 0, st, dcrm, ws + L.dm, rowmap, S0, F, T);
    HIPCHECK(e, hipGetLastError());
    if ((rc = fsn_wgrad(e, L, ws, ws + L.dm, ws + L.hs[1][NL - 1] + S1 * Hs, R1, 2, Hs, gsb[4 * NL], 2, Hs, st))) return rc;
    if ((rc = fsn_bgrad(e, L, ws, ws + L.dm, R1, 2, 2, gsb[4 * NL + 1], nullptr, st))) return rc;
    for (int l = NL - 1; l >= 0; l--) {
        const bool top = l == NL - 1;
        if ((rc = fsn_bptt(e, L, ws, 1, l, top ? nullptr : ws + L.dx, top ? ws + L.dm : nullptr, e->sb.fcw.p, st))) return rc;
        const float *dg = ws + L.dg;
        const float *x = l == 0 ? ws + L.xs[1] : ws + L.hs[1][l - 1] + S1 * Hs;
        const int in = l == 0 ? e->SI : Hs;
        if ((rc = fsn_wgrad(e, L, ws, dg, x, R1, 4 * Hs, in, gsb[4 * l], 4 * Hs, in, st))) return rc;
        if ((rc = fsn_wgrad(e, L, ws, dg, ws + L.hs[1][l], R1, 4 * Hs, Hs, gsb[4 * l + 1], 4 * Hs, Hs, st))) return rc;
        if ((rc = fsn_bgrad(e, L, ws, dg, R1, 4 * Hs, 4 * Hs, gsb[4 * l + 2], gsb[4 * l + 3], st))) return rc;
        if (l > 0) {
            if ((rc = tchk(e, se_train_gemm(dg, e->sb.wih_t[l].p, nullptr, ws + L.dx, (int)R1, Hs, 4 * Hs, 0, st)))) return rc;
        } else {  // d fb_out through the sub-band CumLayerNorm and the full-band ReLU
            HIPCHECK(e, hipMemsetAsync(ws + L.dpre, 0, (size_t)R0 * Fp * sizeof(float), st));
            hipLaunchKernelGGL(k_fsn_dfb, dim3(4096), dim3(256), 0, st, dg, e->sb.wcol.p, ws + L.denom, ws + L.fbo, ws + L.dpre, S0, F, T, 4 * Hs, Fp);
            HIPCHECK(e, hipGetLastError());
        }
    }
    // full band: Linear(H -> F) + ReLU over the last layer, then the layers top down (the input |X| carries no gradient)
    if ((rc = fsn_wgrad(e, L, ws, ws + L.dpre, ws + L.hs[0][NL - 1] + S0 * Hf, R0, Fp, Hf, gfb[4 * NL], F, Hf, st))) return rc;
    if ((rc = fsn_bgrad(e, L, ws, ws + L.dpre, R0, Fp, F, gfb[4 * NL + 1], nullptr, st))) return rc;
    if ((rc = tchk(e, se_train_gemm(ws + L.dpre, e->fb.fcw_t.p, nullptr, ws + L.dx, (int)R0, Hf, Fp, 0, st)))) return rc;
    for (int l = NL - 1; l >= 0; l--) {
        if ((rc = fsn_bptt(e, L, ws, 0, l, ws + L.dx, nullptr, nullptr, st))) return rc;
        const float *dg = ws + L.dg;
        const float *x = l == 0 ? ws + L.xs[0] : ws + L.hs[0][l - 1] + S0 * Hf;
        const int ld = l == 0 ? e->Kp : Hf, in = l == 0 ? e->fb.in : Hf;
        if ((rc = fsn_wgrad(e, L, ws, dg, x, R0, 4 * Hf, ld, gfb[4 * l], 4 * Hf, in, st))) return rc;
        if ((rc = fsn_wgrad(e, L, ws, dg, ws + L.hs[0][l], R0, 4 * Hf, Hf, gfb[4 * l + 1], 4 * Hf, Hf, st))) return rc;
        if ((rc = fsn_bgrad(e, L, ws, dg, R0, 4 * Hf, 4 * Hf, gfb[4 * l + 2], gfb[4 * l + 3], st))) return rc;
        if (l > 0 && (rc = tchk(e, se_train_gemm(dg, e->fb.wih_t[l].p, nullptr, ws + L.dx, (int)R0, Hf, 4 * Hf, 0, st)))) return rc;
    }
    return SE_OK;
}

}  // namespace
