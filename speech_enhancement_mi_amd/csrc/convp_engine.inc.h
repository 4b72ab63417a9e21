// convp_engine.inc.h - engine side of the plane-layout convolution path (conv_p.hip.h); included by se_engine.hip.
//
// Encoder and decoder of TemporalCRN.forward (CRN.py:463-495) with every MFMA operand tensor kept in HBM as split-bf16
// planes ("P layout") and every pre-norm convolution output as channel-octet-innermost fp32 ("R layout"):
//
//   k_featurize_p -> P            4 x ( k_conv_p -> R + statistics ; k_gln_p -> P )      [last level: -> fp32 GRU input]
//   bottleneck (unchanged GEMM / GRU kernels) -> k_gln2_p -> P
//   3 x ( k_conv_p both parities -> R parity-planar ; k_skip_p, or k_conv_p 1x1 statistics pass + 1x1 with fused skip gate -> P )
//   k_conv_p (both parities merged, 4 GEMM rows) -> R ; k_final_mask_p
// (from a waveform: k_stft_feat in place of k_stft + k_featurize_p, k_mask_istft in place of k_final_mask_p + k_istft, io_fused.hip.h)
//
// The ring slot r of encoder level i is xinP[i] + r * slot_elems (ONE allocation per level, so that the history slot is
// addressable through the same buffer descriptor as the current one).

namespace {

struct ConvPPlan {
    ConvPArgs a{};
    int NT = 0, CO = 1, grid_x = 0;
    size_t lds = 0;
    bool active = false;
    DevBuf wx, bias;
    double flops = 0;
    struct Geo { int NT = 0, tpw = 0, n_wg = 0, grouped = 0; size_t lds = 0; long items = 0; } geo[16], gpair[16];
    int ngeo = 0, ngpair = 0;  // gpair: tilings of the k_conv_p<.., NTAP2> instances (a.ntap2 > 0: a second tap list, the odd parity of a
                               // transposed convolution, on the same patch)
    int npair = 0, terms = 6, npair2 = 0;
    PlaneFmt fmt = PlaneFmt::kBf16;  // format of the INPUT planes (and of a P-layout output): which k_conv_p form the launch takes
    int wpl = 3;                     // stored planes of the weight image: the instance's weight-plane parameter
    double flops_pair = 0;
    std::string name;  // launch-site label ("enc3", "skip0", ...): SE_CONVP_NT_<name>=n forces a tiling for experiments
};

struct SkipPPlan {  // k_skip_p: the whole skip gate of one decoder level, one workgroup per stream
    SkipPArgs a{};
    DevBuf wx, cst;
    int KP = 0, wpl = 3;  // K steps; stored planes of the weight image
    size_t lds = 0;
    bool active = false;
    double flops = 0;
};

struct PLevel {
    ConvPPlan enc, dec_even, dec_odd, skip, skipm;
    ConvPPlan gate[2];  // CRN_ELU / student: conv_trans * sigmoid(conv_gated) after the encoder convolution, <= 64 channels per launch
    SkipPPlan sk;
    PlaneFmt sk_fmt = PlaneFmt::kBf16;  // format of res and of the gated output (k_skip_p)
    bool dec_merged = false;
    bool dec_pair_on = false;  // this batch: both parities in one launch of dec_even (a.ntap2 > 0), dec_odd not launched
};

// the planes of one weight in the format of the launch that reads it (conv_weight_image.h: `parts`): the fp16 pair's
// (2^11 w_hi, w_lo, w_hi), one fp16 number, or (hi, mid, lo) bf16
// (PL = the stored planes of the image: the pair's two or three, split_f16pair.h)
inline void weight_parts(float x, int PL, PlaneFmt fmt, uint16_t (&p)[3]) {
    if (fmt == PlaneFmt::kF16Pair) { pair_weight_parts(x, PL, p); return; }
    const uint16_t h = bf16_rne(x);
    const float r1 = x - bf16_to_f32(h);
    const uint16_t md = bf16_rne(r1);
    p[0] = PL == 1 ? f16_rne(x) : h; p[1] = md; p[2] = bf16_rne(r1 - bf16_to_f32(md));
}

}  // namespace

struct se_convp_state {
    PLevel pv[SE_MAX_LEVELS];
    DevBuf xinP[SE_MAX_LEVELS];   // [kRing][B][C8][PL][T][F] uint4
    long slot_elems[SE_MAX_LEVELS]{};  // uint4 per ring slot
    DevBuf encR[SE_MAX_LEVELS];   // [B][Co8][T*Fo][8]
    DevBuf encA[SE_MAX_LEVELS];   // CRN_ELU / student: act(conv) in the P layout, the input of the gated 1x1 pair
    // CRN_ELU / student: the three 5x5 frequency-dilated pre-conv blocks on the plane path (CRN_ELU.py:335-340, 375-376)
    bool pre_p = false;
    ConvPPlan pre[3];
    DevBuf pinP[3];               // block inputs, [kRing][B][1][PL][T][F0] (ring: the previous slot's tail = the 4 history frames)
    long pslot_elems = 0;         // uint4 per ring slot
    DevBuf preR, pre_gw[3];       // gated output of a block, R layout [B][1][T*F0][8]; gate weights of each block
    DevBuf decinP[kRing];         // decoder input, P layout
    DevBuf decR[SE_MAX_LEVELS];   // [B][Co8][T*2Fi][8] parity-planar
    DevBuf decP[SE_MAX_LEVELS];   // blended decoder level outputs, P layout
    PlaneFmt ring_fmt = PlaneFmt::kBf16;  // format of what xinP[i >= 1] holds (alloc_state_p, convert_history_p)
    ConvPPlan tap_enc;            // CRN_ELU / student, feature tap ft0: the last encoder convolution once more, writing the R layout
                                  // (tap_enc_plan: built on first use, dropped by prepare_weights_p)
    bool ready = false;
};

namespace {

template <class WSel>
int plan_conv_p(se_engine *e, ConvPPlan &pl, int Ci, int Co, int FP, int Fi, int s, int colpad, int tlo_off, int ngroup, int dil, int St,
                const std::vector<std::array<int, 4>> &taps, WSel wsel, const std::vector<float> &bias_logical, int relu_lo, int relu_hi,
                int act, int out_mode, PlaneFmt fmt = PlaneFmt::kBf16) {
    pl.active = FP > 0;
    pl.fmt = fmt;
    if (!pl.active) return 0;
    // PL: stored weight planes (the pair's two, or three under SE_PAIR_W3); APL: planes of the patch this launch stages
    const bool fpair = fmt == PlaneFmt::kF16Pair;
    const int T = e->T, ntap = (int)taps.size(), PL = fpair ? pair_wplanes(e) : operand_planes(e->precision), APL = fpair ? kPairPlanesA : operand_planes(e->precision);
    pl.wpl = PL;
    const int P = T * FP, tiles = (P + 31) / 32;
    const int CoPad = (Co + 31) / 32 * 32;
    if (CoPad > 128 || CoPad == 96) return fail(e, SE_ERR_ARG, "conv with %d GEMM rows is not supported", Co);
    const int MT = CoPad / 32, NCG = 4 / MT;
    const int C8 = (Ci + 7) / 8;
    int CO = 1;
    if (ntap == 1) CO = C8 >= 4 ? 4 : (C8 >= 2 ? 2 : 1);
    if (C8 % CO) return fail(e, SE_ERR_ARG, "channel octets %d not a multiple of the chunk %d", C8, CO);
    const int nchunk = C8 / CO, npair = (ntap * CO + 1) / 2;
    pl.ngeo = pl.ngpair = 0;
    static const int nts[] = {1, 2, 3, 4, 6, 8, 10, 12};
    for (int nt : nts) {
        const bool single = conv_p_has_instance(ntap, nt, CO), pair = pl.a.ntap2 && conv_p_has_instance(ntap, nt, CO, pl.a.ntap2);
        if (!single && !pair) continue;
        const int tpw_max = NCG * nt;
        const int n_wg = (tiles + tpw_max - 1) / tpw_max;
        const int tpw = (tiles + n_wg - 1) / n_wg;
        if ((tpw + NCG - 1) / NCG != nt) continue;  // a smaller instance covers this tiling
        int rows_pos = (tpw * 32 + FP - 1) / FP + 1;
        if (rows_pos > T) rows_pos = T;
        const int grouped = ngroup * rows_pos < rows_pos + (ngroup - 1) * dil;
        const int Rmax = grouped ? ngroup * rows_pos : rows_pos + (ngroup - 1) * dil;
        const long items = (long)APL * CO * Rmax * St;
        if (items > 256L * kPNiMax) continue;
        // whole LDS-DMA instructions: the last one may write zero pieces past `items`, so the allocation covers NI * 256 pieces
        const size_t lds = (size_t)((items + 255) / 256) * 4096;
        if (lds > 160 * 1024) continue;
        const ConvPPlan::Geo g{nt, tpw, n_wg, grouped, lds, items};
        if (single) pl.geo[pl.ngeo++] = g;
        if (pair) pl.gpair[pl.ngpair++] = g;
    }
    if (!pl.ngeo) return fail(e, SE_ERR_ARG, "no conv_p tiling fits (taps %d, Ci %d, Co %d, FP %d, St %d)", ntap, Ci, Co, FP, St);
    ConvPArgs &a = pl.a;
    a.C8 = C8; a.Ci = Ci; a.Co = Co; a.CoPad = CoPad; a.T = T; a.Fi = Fi; a.FP = FP;
    a.s = s; a.colpad = colpad; a.tlo_off = tlo_off; a.ngroup = ngroup; a.dil = dil; a.ntap = ntap;
    a.deint = s == 2 ? 1 : 0;
    a.Sh = (St + 1) / 2;
    for (int t = 0; t < ntap; t++) {
        a.rowgrp[t] = taps[t][2];
        const int c = taps[t][3];
        a.coloff[t] = a.deint ? (c & 1) * a.Sh + (c >> 1) : c;
    }
    a.nchunk = nchunk; a.St = St; a.act = act; a.relu_lo = relu_lo; a.relu_hi = relu_hi;
    a.out_mode = out_mode; a.row_perm = out_mode == kPOutP || out_mode == kPOutBlend || out_mode == kPOutGate;
    a.valid_m = FP; a.par_rows = 0; a.stats = nullptr;
    pl.npair2 = a.ntap2 ? (a.ntap2 * CO + 1) / 2 : 0;
    pl.CO = CO; pl.npair = npair; pl.terms = fmt == PlaneFmt::kF16Pair ? 3 : (PL == 3 ? 6 : (PL == 2 ? 3 : 1));
    // weights [chunk][pair][plane][mtile][row 32][k 16] (conv_weight_image.h), the planes of a weight in the launch's format
    const std::vector<uint16_t> wx = convp_weight_image(out_mode, CO, nchunk, Ci, Co, CoPad, PL, taps, wsel,
                                                        [=](float x, uint16_t (&p)[3]) { weight_parts(x, PL, fmt, p); });
    std::vector<float> bias(CoPad, 0.0f);
    for (int row = 0; row < CoPad; row++) {
        const int lg = convp_row_logical(out_mode, row);
        if (lg < Co) bias[row] = bias_logical[lg];
    }
    int rc = dev_alloc(e, pl.wx, (wx.size() + 1) / 2);
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(pl.wx.p, wx.data(), wx.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    a.wx = reinterpret_cast<const uint4 *>(pl.wx.p);
    if ((rc = dev_upload(e, pl.bias, bias))) return rc;
    a.bias = pl.bias.p;
    return 0;
}

// Picks the tiling for the current batch: time ~ rounds x (workgroups per CU x MFMA cycles + staging + epilogue).  pair: among the
// tilings of the two-parity instances.  Returns the modelled cost.
double select_convp_geometry(se_engine *e, ConvPPlan &pl, bool pair = false) {
    if (!pl.active) return 0;
    const ConvPPlan::Geo *geo = pair ? pl.gpair : pl.geo;
    const int ngeo = pair ? pl.ngpair : pl.ngeo, npair2 = pair ? pl.npair2 : 0;
    double best = 0;
    int pick = -1;
    int force = getenv("SE_CONVP_NT") ? atoi(getenv("SE_CONVP_NT")) : 0;
    if (const char *s = getenv(("SE_CONVP_NT_" + pl.name).c_str())) force = atoi(s);
    for (int k = 0; k < ngeo; k++) {
        const ConvPPlan::Geo &g = geo[k];
        const int nacc = npair2 ? 2 * g.NT : g.NT;  // accumulator sets x tiles
        const int wgpc = (nacc <= 6 && g.lds <= 80 * 1024) ? 2 : 1;  // k_conv_p<.., NT <= 6> is built for two workgroups per CU
        const double rounds = std::ceil((double)g.n_wg * e->B / ((double)e->num_cu * wgpc));
        const double mfma = (double)pl.a.nchunk * (pl.npair + npair2) * g.NT * pl.terms * 32.0;
        const double stage = (double)pl.a.nchunk * g.items * 1.0 + pl.a.nchunk * 2500.0;  // ~16 B/cycle/CU + DMA latency and barriers per chunk
        const double epi = nacc * 600.0 + (npair2 ? 2 : 1) * 3000.0;
        const double cost = rounds * (wgpc * mfma + stage + epi);
        if (pick < 0 || cost < best) { best = cost; pick = k; }
        if (force && g.NT == force) { pick = k; best = cost; break; }
    }
    if (pick < 0 || (pair && force && geo[pick].NT != force)) return 1e300;  // (a pinned tiling the pair instances lack: two launches)
    const ConvPPlan::Geo &g = geo[pick];
    if (getenv("SE_CONVP_VERBOSE")) {
        fprintf(stderr, "[conv_p] %-10s taps %2d%s Ci %3d rows %3d FP %3d: NT %2d tiles/wg %2d wgs/stream %2d lds %6zu items %5ld chunks %d pairs %d cost %.0f | candidates:", pl.name.c_str(),
                pl.a.ntap, pair ? "+6" : "", pl.a.Ci, pl.a.Co, pl.a.FP, g.NT, g.tpw, g.n_wg, g.lds, g.items, pl.a.nchunk, pl.npair + npair2, best);
        for (int k = 0; k < ngeo; k++) fprintf(stderr, " %d", geo[k].NT);
        fprintf(stderr, "\n");
    }
    pl.NT = g.NT; pl.grid_x = g.n_wg; pl.lds = g.lds;
    pl.a.tiles_per_wg = g.tpw; pl.a.grouped = g.grouped;
    return best;
}

#ifdef SE_CP_TRACE
struct CpTraceSites {
    std::vector<std::pair<std::string, unsigned long long *>> sites;
    unsigned long long *get(const char *label, int NT, int grid_x) {
        const std::string key = std::string(label ? label : "?") + " NT=" + std::to_string(NT) + " wg/stream=" + std::to_string(grid_x);
        for (auto &s : sites) if (s.first == key) return s.second;
        unsigned long long *p = nullptr;
        (void)hipMalloc(&p, 64); (void)hipMemset(p, 0, 64);
        sites.emplace_back(key, p);
        return p;
    }
    void dump() {
        for (auto &s : sites) {
            unsigned long long h[8];
            if (hipMemcpy(h, s.second, sizeof h, hipMemcpyDeviceToHost) != hipSuccess || !h[7]) continue;
            const double n = (double)h[7];
            fprintf(stderr, "[cp trace %-34s] %8llu WGs, cycles/WG: prologue %7.0f  barrier1 %7.0f  dma issue %7.0f  barrier2+dma wait %7.0f  mfma loop %7.0f  epilogue %7.0f\n",
                    s.first.c_str(), h[7], h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[5] / n);
            (void)hipMemset(s.second, 0, 64);
        }
    }
};
static CpTraceSites g_cp_trace_sites;
#endif

int launch_conv_p(se_engine *e, const ConvPPlan &pl, const ConvPArgs &a_in, hipStream_t st, const char *label) {
    if (!pl.active) return 0;
    ProfScope ps(e, "k_conv_p", label, (a_in.ntap2 ? pl.flops_pair : pl.flops) * e->B, st);
    ConvPArgs a = a_in;
    a.trace = nullptr;
#ifdef SE_CP_TRACE
    a.trace = g_cp_trace_sites.get(label, pl.NT, pl.grid_x);
#endif
    if (conv_p_launch(a.ntap, a.ntap2, pl.NT, pl.CO, pl.wpl, dim3(pl.grid_x, e->Bact), pl.lds, st, a, pl.fmt))
        return fail(e, SE_ERR_ARG, "no conv_p kernel instance for %d (+ %d) taps x %d tiles x %d octets", a.ntap, a.ntap2, pl.NT, pl.CO);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// statistics slots of a decoder level's odd parity: its own launch, the second half of a pair launch, or none (last level)
int dec_odd_slots(const PLevel &pv) { return pv.dec_pair_on ? pv.dec_even.grid_x : (pv.dec_odd.active ? pv.dec_odd.grid_x : 0); }

uint4 *decin_p(se_engine *e, int slot) { return reinterpret_cast<uint4 *>(e->cp->decinP[slot].p); }

// uint4 per stream of xinP[i] in its current format: the stream stride inside a ring slot (the slot itself, slot_elems, stays sized
// for the bf16 planes: a later weight load may fail the range guard and switch the format back without a re-plan of the batch)
long xin_stream_elems(const se_engine *e, int i) { return (long)((e->Ch[i] + 7) / 8) * act_planes(e, xin_kind(i)) * e->T * e->F[i]; }

void select_all_p(se_engine *e) {
    for (int i = 0; i < e->L; i++) {
        PLevel &pv = e->cp->pv[i];
        for (ConvPPlan *p : {&pv.enc, &pv.skip, &pv.skipm, &pv.gate[0], &pv.gate[1]}) select_convp_geometry(e, *p);
        // a decoder level runs its two parities in one launch where the model prices that below the two launches of this batch.
        // The model prices the rounds of a launch, not its start and drain (about 5 us, 12000 cycles, which no workgroup count hides):
        // the same for every tiling of one launch, but the two-launch form pays it twice.  Without it the 512-point dec2 at B = 256
        // was priced 0.7 % below its pair launch and measured 69.3 us against 57.8 us.
        constexpr double kLaunchCycles = 12000.0;
        pv.dec_pair_on = false;
        if (pv.dec_even.active && pv.dec_even.a.ntap2 && pv.dec_even.ngpair) {
            const double two = select_convp_geometry(e, pv.dec_even) + select_convp_geometry(e, pv.dec_odd) + kLaunchCycles;
            ConvPPlan::Geo keep{pv.dec_even.NT, pv.dec_even.a.tiles_per_wg, pv.dec_even.grid_x, pv.dec_even.a.grouped, pv.dec_even.lds, 0};
            const double one = select_convp_geometry(e, pv.dec_even, true);
            if (e->dec_pair_site[i] >= 0 ? e->dec_pair_site[i] == 1 : one < two) pv.dec_pair_on = true;  // (SE_DEC_PAIR_dec<i> beats the model)
            else { pv.dec_even.NT = keep.NT; pv.dec_even.a.tiles_per_wg = keep.tpw; pv.dec_even.grid_x = keep.n_wg; pv.dec_even.a.grouped = keep.grouped; pv.dec_even.lds = keep.lds; }
        } else {
            select_convp_geometry(e, pv.dec_even);
            select_convp_geometry(e, pv.dec_odd);
        }
    }
    if (e->cp->pre_p)
        for (int i = 0; i < e->npre; i++) select_convp_geometry(e, e->cp->pre[i]);
}

void free_state_p(se_engine *e) {
    if (!e->cp) return;
    se_convp_state &S = *e->cp;
    for (int i = 0; i < SE_MAX_LEVELS; i++) {
        for (ConvPPlan *p : {&S.pv[i].enc, &S.pv[i].dec_even, &S.pv[i].dec_odd, &S.pv[i].skip, &S.pv[i].skipm, &S.pv[i].gate[0], &S.pv[i].gate[1]}) { dev_free(p->wx); dev_free(p->bias); }
        dev_free(S.pv[i].sk.wx); dev_free(S.pv[i].sk.cst);
        dev_free(S.xinP[i]); dev_free(S.encR[i]); dev_free(S.encA[i]); dev_free(S.decR[i]); dev_free(S.decP[i]);
    }
    for (int r = 0; r < kRing; r++) dev_free(S.decinP[r]);
    for (int i = 0; i < 3; i++) { dev_free(S.pre[i].wx); dev_free(S.pre[i].bias); dev_free(S.pinP[i]); dev_free(S.pre_gw[i]); }
    dev_free(S.preR); dev_free(S.tap_enc.wx); dev_free(S.tap_enc.bias);
    delete e->cp;
    e->cp = nullptr;
}

// The strided convolution of encoder level i (CRN.py:331-336) as a k_conv_p plan that writes `out_mode`
int plan_enc_conv_p(se_engine *e, int i, ConvPPlan &pl, int out_mode) {
    const int Ci = e->Ch[i], Co = e->Ch[i + 1], Fi = e->F[i], Fo = e->F[i + 1], d = 1 << i, T = e->T;
    const std::string p = "convlist." + std::to_string(i) + ".";
    auto *w = param(e, p + "conv.weight", (size_t)Co * Ci * 15);
    auto *b = param(e, p + "conv.bias", Co);
    if (!w || !b) return SE_ERR_PARAM_MISSING;
    std::vector<std::array<int, 4>> taps;
    for (int kf = 0; kf < 5; kf++)
        for (int kt = 0; kt < 3; kt++) taps.push_back({kf, kt, kt, kf});
    const float *wp = w->data();
    int rc = plan_conv_p(e, pl, Ci, Co, Fo, Fi, 2, 2, -2 * d, 3, d, Fi + 4, taps,
                         [=](int ci, int co, int kf, int kt) { return wp[(((size_t)co * Ci + ci) * 5 + kf) * 3 + kt]; }, *b, 0, Co, e->act,
                         out_mode, act_format(e, xin_kind(i)));  // (level 0 reads the features: bf16 planes)
    if (rc) return rc;
    ConvPArgs &a = pl.a;
    a.oT = Fo; a.oo = 0; a.y_npos = T * Fo; a.y_stream = (long)((Co + 7) / 8) * T * Fo * 8;
    a.stats_lo = 0; a.stats_hi = Co;
    pl.flops = 2.0 * Co * Ci * 15 * Fo * T;
    return 0;
}

// Feature tap ft0 re-runs the last encoder convolution into the R layout.  The CRN's own plan writes that; CRN_ELU / the student write
// act(conv) as planes with permuted GEMM rows, so their tap keeps a twin of the plan, tiled for the current batch.
int tap_enc_plan(se_engine *e, const ConvPPlan **out) {
    se_convp_state &S = *e->cp;
    const int i = e->L - 1;
    *out = &S.pv[i].enc;
    if (!e->variant) return 0;
    if (!S.tap_enc.active) {
        int rc = plan_enc_conv_p(e, i, S.tap_enc, kPOutR);
        if (rc) return rc;
        S.tap_enc.name = "tap_enc";
    }
    select_convp_geometry(e, S.tap_enc);
    *out = &S.tap_enc;
    return 0;
}

int prepare_weights_p(se_engine *e) {
    se_convp_state &S = *e->cp;
    const int L = e->L, T = e->T;
    S.tap_enc.active = false;  // planned from the previous weights
    // The pre-conv blocks run on k_conv_p only with fp16 operands: a workgroup stages a 6-7 row x (F + 4 fd) column patch for
    // 1-2 output rows, and with three bf16 planes that staging costs more than the scalar-weight vector-ALU kernel takes
    // (measured, student B = 1024: 760 vs 450 us per block in f32, equal in bf16x3, 0.6x in fp16).  SE_PRE_P=0/1 overrides.
    S.pre_p = e->npre > 0 && (getenv("SE_PRE_P") ? atoi(getenv("SE_PRE_P")) != 0 : operand_planes(e->precision) == 1);
    for (int i = 0; i < e->npre && S.pre_p; i++) {  // Conv2d(5x5, dilation (fd,1), padding (2fd,4)) + ELU + gated pair (CRN_ELU.py:335-340)
        const int C0 = e->Ch[0], F0 = e->F[0], fd = 1 << i;
        const std::string p = "preconvlist." + std::to_string(i) + ".";
        auto *w = param(e, p + "conv.weight", (size_t)C0 * C0 * 25);
        auto *b = param(e, p + "conv.bias", C0);
        auto *tw = param(e, p + "conv_trans.weight", (size_t)C0 * C0);
        auto *tb = param(e, p + "conv_trans.bias", C0);
        auto *gw = param(e, p + "conv_gated.weight", (size_t)C0 * C0);
        auto *gb = param(e, p + "conv_gated.bias", C0);
        if (!w || !b || !tw || !tb || !gw || !gb) return SE_ERR_PARAM_MISSING;
        std::vector<std::array<int, 4>> taps;
        for (int kf = 0; kf < 5; kf++)
            for (int kt = 0; kt < 5; kt++) taps.push_back({kf, kt, kt, kf * fd});
        const float *wp = w->data();
        int rc = plan_conv_p(e, S.pre[i], C0, C0, F0, F0, 1, 2 * fd, -4, 5, 1, F0 + 4 * fd, taps,
                             [=](int ci, int co, int kf, int kt) { return wp[(((size_t)co * C0 + ci) * 5 + kf) * 5 + kt]; }, *b, 0, C0, 2, kPOutPre);
        if (rc) { S.pre_p = false; e->err.clear(); break; }  // (no tiling fits: the blocks stay on the fp32 vector-ALU kernel)
        S.pre[i].name = "pre" + std::to_string(i);
        ConvPArgs &a = S.pre[i].a;
        a.Cy = C0; a.oT = F0; a.oo = 0; a.y_npos = T * F0; a.y_stream = (long)T * F0 * 8;
        std::vector<float> g;
        g.insert(g.end(), tw->begin(), tw->end());
        g.insert(g.end(), gw->begin(), gw->end());
        g.insert(g.end(), tb->begin(), tb->end());
        g.insert(g.end(), gb->begin(), gb->end());
        if ((rc = dev_upload(e, S.pre_gw[i], g))) return rc;
        a.gatew = S.pre_gw[i].p;
        S.pre[i].flops = 2.0 * C0 * C0 * 25 * F0 * T + 2.0 * 2 * C0 * C0 * F0 * T;
    }
    for (int i = 0; i < L; i++) {
        const int Co = e->Ch[i + 1], Fo = e->F[i + 1];
        const std::string p = "convlist." + std::to_string(i) + ".";
        int rc = plan_enc_conv_p(e, i, S.pv[i].enc, e->variant ? kPOutP : kPOutR);
        if (rc) return rc;
        S.pv[i].enc.name = "enc" + std::to_string(i);
        ConvPArgs &a = S.pv[i].enc.a;
        S.pv[i].gate[0].active = S.pv[i].gate[1].active = false;
        if (e->variant) {  // act(conv) -> P layout -> gated 1x1 pair (CRN_ELU.py:223-224, 240) -> R layout + statistics
            a.Cy = Co; a.Fy = Fo; a.yp_stream = (long)((Co + 7) / 8) * operand_planes(e->precision) * T * Fo;
            auto *tw = param(e, p + "conv_trans.weight", (size_t)Co * Co);
            auto *tb = param(e, p + "conv_trans.bias", Co);
            auto *gw = param(e, p + "conv_gated.weight", (size_t)Co * Co);
            auto *gb = param(e, p + "conv_gated.bias", Co);
            if (!tw || !tb || !gw || !gb) return SE_ERR_PARAM_MISSING;
            const float *twp = tw->data(), *gwp = gw->data();
            const int nparts = Co > 64 ? 2 : 1, cpart = ((Co + nparts - 1) / nparts + 7) / 8 * 8;
            std::vector<std::array<int, 4>> t1 = {{0, 0, 0, 0}};
            for (int part = 0; part < nparts; part++) {
                const int c0 = part * cpart, cn = std::min(cpart, Co - c0);
                std::vector<float> bias2(2 * cn);
                for (int c = 0; c < cn; c++) { bias2[2 * c] = (*tb)[c0 + c]; bias2[2 * c + 1] = (*gb)[c0 + c]; }
                ConvPPlan &g = S.pv[i].gate[part];
                if ((rc = plan_conv_p(e, g, Co, 2 * cn, Fo, Fo, 1, 0, 0, 1, 0, Fo, t1,
                                      [=](int ci, int row, int, int) { const int c = c0 + row / 2; return (row & 1) ? gwp[(size_t)c * Co + ci] : twp[(size_t)c * Co + ci]; },
                                      bias2, 0, 0, 0, kPOutGate))) return rc;
                g.name = "gate" + std::to_string(i);
                g.a.Cy = cn; g.a.gate_c0 = c0; g.a.oT = Fo; g.a.oo = 0; g.a.y_npos = T * Fo; g.a.y_stream = a.y_stream;
                g.flops = 2.0 * 2 * cn * Co * Fo * T;
            }
        }
    }
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j;
        const int Ci = e->Ch[lvl + 1], Co = lvl == 0 ? 2 : e->Ch[lvl], Fi = e->F[lvl + 1], d = 1 << j;
        const std::string p = "deconvlist." + std::to_string(j) + ".";
        auto *w = param(e, p + "conv.weight", (size_t)Co * Ci * 15);
        auto *b = param(e, p + "conv.bias", Co);
        if (!w || !b) return SE_ERR_PARAM_MISSING;
        const float *wp = w->data();
        auto wsel = [=](int ci, int co, int kf, int kt) { return wp[(((size_t)ci * Co + co) * 5 + kf) * 3 + kt]; };
        PLevel &pv = S.pv[j];
        const PlaneFmt cfmt = act_format(e, PlaneBuf::kConvAct);  // decinP / decP in, xinP[lvl] in and decP out on the skip path
        int rc;
        pv.dec_even.name = "dec" + std::to_string(j) + "_even"; pv.dec_odd.name = "dec" + std::to_string(j) + "_odd";
        pv.skip.name = "skip" + std::to_string(j); pv.skipm.name = "skipstat" + std::to_string(j);
        pv.dec_even.a.ntap2 = 0;
        pv.dec_merged = lvl == 0;  // the last block (2 mask channels): both parities as 4 GEMM rows of ONE launch
        if (pv.dec_merged) {
            std::vector<std::array<int, 4>> tu;
            for (int kf = 0; kf < 5; kf++)
                for (int kt = 0; kt < 3; kt++) tu.push_back({kf, kt, 2 - kt, (kf & 1) ? 1 + (3 - kf) / 2 : 2 - kf / 2});
            std::vector<float> bias2(2 * Co);
            for (int c = 0; c < Co; c++) bias2[2 * c] = bias2[2 * c + 1] = (*b)[c];
            rc = plan_conv_p(e, pv.dec_even, Ci, 2 * Co, Fi, Fi, 1, 1, 0, 3, d, Fi + 2, tu,
                             [=](int ci, int row, int kf, int kt) { return ((row & 1) == (kf & 1)) ? wsel(ci, row >> 1, kf, kt) : 0.0f; },
                             bias2, 0, 2 * Co, e->act, kPOutR, cfmt);
            if (rc) return rc;
            ConvPArgs &a = pv.dec_even.a;
            a.par_rows = 1; a.oT = Fi; a.oo = 0; a.y_npos = T * Fi; a.y_stream = (long)T * Fi * 8;
            a.stats_lo = 0; a.stats_hi = 2 * Co;
            pv.dec_even.flops = 2.0 * Ci * Co * 15 * Fi * T;
            pv.dec_odd.active = false;
        } else {
            std::vector<std::array<int, 4>> te, to;
            for (int kf = 0; kf < 5; kf += 2)
                for (int kt = 0; kt < 3; kt++) te.push_back({kf, kt, 2 - kt, 2 - kf / 2});
            for (int kf = 1; kf < 5; kf += 2)
                for (int kt = 0; kt < 3; kt++) to.push_back({kf, kt, 2 - kt, 1 + (3 - kf) / 2});
            // e->dec_pair: ONE launch (k_conv_p<9, NT, 1, PL, 6>) can stage each chunk of the patch once for both parities; the odd
            // parity then runs over the even one's Fi positions per row and drops m = Fi - 1 (valid_m2).  select_all_p decides per
            // batch (PLevel::dec_pair_on); otherwise two launches.
            // Not with one fp16 plane: there the single-parity kernels are small enough to share a CU with more workgroups than
            // the model counts, and the pair launch measured 2 % slower (student, B = 1024, fp16).
            const bool pair = e->dec_pair && operand_planes(e->precision) >= 2;
            pv.dec_even.a.ntap2 = pair ? (int)to.size() : 0;  // before planning: plan_conv_p then also lists the pair tilings
            if ((rc = plan_conv_p(e, pv.dec_even, Ci, Co, Fi, Fi, 1, 1, 0, 3, d, Fi + 2, te, wsel, *b, 0, Co, e->act, kPOutR, cfmt))) return rc;
            if ((rc = plan_conv_p(e, pv.dec_odd, Ci, Co, Fi - 1, Fi, 1, 1, 0, 3, d, Fi + 2, to, wsel, *b, 0, Co, e->act, kPOutR, cfmt))) return rc;
            for (ConvPPlan *q : {&pv.dec_even, &pv.dec_odd}) {
                ConvPArgs &a = q->a;
                a.oT = 2 * Fi; a.oo = q == &pv.dec_odd ? Fi : 0; a.y_npos = T * 2 * Fi; a.y_stream = (long)((Co + 7) / 8) * T * 2 * Fi * 8;
                a.stats_lo = 0; a.stats_hi = Co;
            }
            pv.dec_even.flops = 2.0 * Ci * Co * 9 * Fi * T;
            pv.dec_odd.flops = 2.0 * Ci * Co * 6 * Fi * T;
            if (pair) {  // the odd parity's taps and weights (same chunks, CO = 1) ride along in the even plan
                ConvPArgs &a = pv.dec_even.a;
                const ConvPArgs &o = pv.dec_odd.a;
                if (o.nchunk != a.nchunk || o.CoPad != a.CoPad) return fail(e, SE_ERR_ARG, "decoder parities of level %d do not share chunks", j);
                for (int t = 0; t < o.ntap; t++) { a.rowgrp2[t] = o.rowgrp[t]; a.coloff2[t] = o.coloff[t]; }
                a.wx2 = o.wx; a.oo2 = Fi; a.valid_m2 = Fi - 1;
                pv.dec_even.flops_pair = pv.dec_even.flops + pv.dec_odd.flops;
            }
        }
        if (lvl > 0) {  // skip path (CRN.py:387-396): statistics pass of residualmask + the gated 1x1 pair
            auto *mw = param(e, p + "residualmask.weight", (size_t)Co * Co);
            auto *mb = param(e, p + "residualmask.bias", Co);
            auto *rw = param(e, p + "residual.weight", (size_t)Co * Co);
            auto *rb = param(e, p + "residual.bias", Co);
            if (!mw || !mb || !rw || !rb) return SE_ERR_PARAM_MISSING;
            const float *mwp = mw->data(), *rwp = rw->data();
            std::vector<std::array<int, 4>> t1 = {{0, 0, 0, 0}};
            const int Fr = e->F[lvl];
            std::vector<float> biasp(2 * Co);
            for (int c = 0; c < Co; c++) { biasp[2 * c] = (*mb)[c]; biasp[2 * c + 1] = (*rb)[c]; }
            if ((rc = plan_conv_p(e, pv.skip, Co, 2 * Co, Fr, Fr, 1, 0, 0, 1, 0, Fr, t1,
                                  [=](int ci, int row, int, int) { const int c = row >> 1; return (row & 1) ? rwp[(size_t)c * Co + ci] : mwp[(size_t)c * Co + ci]; },
                                  biasp, 0, 0, e->act, kPOutBlend, cfmt))) return rc;
            if ((rc = plan_conv_p(e, pv.skipm, Co, Co, Fr, Fr, 1, 0, 0, 1, 0, Fr, t1,
                                  [=](int ci, int co, int, int) { return mwp[(size_t)co * Co + ci]; }, *mb, 0, 0, e->act, kPOutR, cfmt))) return rc;
            pv.skipm.a.stats_lo = 0; pv.skipm.a.stats_hi = Co; pv.skipm.a.oT = Fr; pv.skipm.a.oo = 0; pv.skipm.a.y_npos = T * Fr;
            pv.skip.a.Cy = Co; pv.skip.a.Fy = Fr; pv.skip.a.oo = 0;
            pv.skip.flops = 2.0 * 2 * Co * Co * Fr * T;
            pv.skipm.flops = 0;  // recomputation, not algorithmic work
            {   // streaming form (k_skip_p): M tiles [0, MTh) = residualmask, [MTh, 2 MTh) = residual; rows permuted like kPOutP
                auto *mnw = param(e, p + "residualnorm.weight", Co);
                auto *mnb = param(e, p + "residualnorm.bias", Co);
                auto *nw = param(e, p + "norm.weight", Co);
                auto *nb = param(e, p + "norm.bias", Co);
                if (!mnw || !mnb || !nw || !nb) return SE_ERR_PARAM_MISSING;
                SkipPPlan &sk = pv.sk;
                const int PL = cfmt == PlaneFmt::kF16Pair ? pair_wplanes(e) : operand_planes(e->precision);  // stored weight planes
                const int C8 = (Co + 7) / 8, MTh = (Co + 31) / 32, KP = (C8 + 1) / 2, Cp = MTh * 32;
                const int APL = cfmt == PlaneFmt::kF16Pair ? kPairPlanesA : PL;  // planes of res and of the gated output
                sk.wpl = PL;
                pv.sk_fmt = cfmt;
                sk.active = MTh <= 2 && (KP == 1 || KP == 2 || KP == 4);
                if (sk.active) {
                    const std::vector<uint16_t> wx = skip_weight_image(Co, MTh, KP, PL, mwp, rwp, [=](float x, uint16_t (&p)[3]) { weight_parts(x, PL, cfmt, p); });
                    if ((rc = dev_alloc(e, sk.wx, (wx.size() + 1) / 2))) return rc;
                    HIPCHECK(e, hipMemcpy(sk.wx.p, wx.data(), wx.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
                    std::vector<float> cst((size_t)6 * Cp, 0.0f);
                    for (int c = 0; c < Co; c++) {  // [octet][constant][8]: a lane reads one constant of its octet as two 16-byte pieces
                        float *row = &cst[(size_t)(c >> 3) * 6 * 8 + (c & 7)];
                        row[0] = (*mb)[c]; row[8] = (*rb)[c]; row[16] = (*nw)[c]; row[24] = (*nb)[c];
                        row[32] = (*mnw)[c]; row[40] = (*mnb)[c];
                    }
                    if ((rc = dev_upload(e, sk.cst, cst))) return rc;
                    SkipPArgs &a = sk.a;
                    a.C = Co; a.C8 = C8; a.T = T; a.Fr = Fr; a.TF = T * Fr; a.MTh = MTh; a.KP = KP; a.act = e->act;
                    a.wx = reinterpret_cast<const uint4 *>(sk.wx.p); a.cst = sk.cst.p;
                    a.x_stream = (long)C8 * APL * T * Fr; a.out_stream = a.x_stream;
                    a.Fh = Fi; a.Fo = 2 * Fi - 1; a.y_stream = pv.dec_even.a.y_stream; a.eps_mode = e->eps_mode;
                    sk.KP = KP;
                    sk.lds = (size_t)2 * MTh * KP * PL * 64 * 16 + (size_t)6 * Cp * 4;
                    sk.flops = pv.skip.flops;
                }
            }
        } else {
            pv.skip.active = pv.skipm.active = false;
        }
    }
    S.ready = true;
    return 0;
}

// Statistics slabs of the norms (se_engine::enc_stats / dec_stats / skip_stats): one (sum, sum of squares) slot per workgroup of THIS
// selection's grids.  The tiling - and with it grid_x - depends on the buffer format (patch bytes, MFMA terms), so a weight load that
// flips the format of a running batch re-selects and must come back here: called from alloc_state_p and after every select_all_p of
// ensure_ready.  Grows only; a slab is written and read within one segment, so a re-allocation between calls loses nothing.
int alloc_stats_p(se_engine *e) {
    se_convp_state &S = *e->cp;
    const size_t B = (size_t)e->B;
    int rc;
    for (int i = 0; i < e->L; i++) {
        PLevel &pv = S.pv[i];
        if ((rc = dev_alloc(e, e->enc_stats[i], B * 2 * (pv.enc.grid_x + (pv.gate[0].active ? pv.gate[0].grid_x : 0) + (pv.gate[1].active ? pv.gate[1].grid_x : 0) + 1)))) return rc;
        if ((rc = dev_alloc(e, e->dec_stats[i], B * 2 * (pv.dec_even.grid_x + dec_odd_slots(pv) + 1)))) return rc;
        if ((rc = dev_alloc(e, e->skip_stats[i], B * 2 * ((pv.skipm.active ? pv.skipm.grid_x : 0) + 1)))) return rc;
    }
    return 0;
}

// every launch that writes or reads a slab with `nslot` slots per stream checks it against the allocation first
int slab_fits(se_engine *e, const DevBuf &slab, int nslot, const char *what) {
    if ((size_t)e->B * nslot * 2 <= slab.n) return 0;
    return fail(e, SE_ERR_STATE, "statistics slab of %s holds %zu floats, this tiling needs %zu (batch %d x %d slots)", what, slab.n, (size_t)e->B * nslot * 2, e->B, nslot);
}

int alloc_state_p(se_engine *e, hipStream_t st) {
    se_convp_state &S = *e->cp;
    S.ring_fmt = act_format(e, PlaneBuf::kConvAct);  // (the all-zero history is the same bits in both formats)
    const int L = e->L, T = e->T, B = e->B, PL = operand_planes(e->precision);
    int rc;
    for (int i = 0; i < L; i++) {
        const long per = (long)((e->Ch[i] + 7) / 8) * PL * T * e->F[i];  // uint4 per stream
        S.slot_elems[i] = per * B;
        const size_t bytes = (size_t)S.slot_elems[i] * kRing * 16;
        if (bytes >= (size_t)0xFFFFFF00u) return fail(e, SE_ERR_ARG, "activation ring of level %d needs %zu bytes: beyond one buffer descriptor (batch too large)", i, bytes);
        if ((rc = dev_alloc(e, S.xinP[i], bytes / 4))) return rc;
        HIPCHECK(e, hipMemsetAsync(S.xinP[i].p, 0, (size_t)S.slot_elems[i] * 16, st));  // slot 0 = the all-zero history of the first segment
        const int Co = e->Ch[i + 1], Fo = e->F[i + 1];
        if ((rc = dev_alloc(e, S.encR[i], (size_t)B * ((Co + 7) / 8) * T * Fo * 8))) return rc;
        // channel slots beyond Co of the last octet are never written; consumers scale them by zero, so they must be finite
        HIPCHECK(e, hipMemsetAsync(S.encR[i].p, 0, (size_t)B * ((Co + 7) / 8) * T * Fo * 8 * sizeof(float), st));
        if (e->variant && (rc = dev_alloc(e, S.encA[i], (size_t)B * ((Co + 7) / 8) * PL * T * Fo * 4))) return rc;
    }
    for (int r = 0; r < kRing; r++)
        if ((rc = dev_alloc(e, S.decinP[r], (size_t)B * ((e->Ch[L] + 7) / 8) * PL * T * e->F[L] * 4))) return rc;
    if (S.pre_p) {
        S.pslot_elems = (long)PL * T * e->F[0] * B;
        for (int i = 0; i < e->npre; i++) {
            if ((rc = dev_alloc(e, S.pinP[i], (size_t)S.pslot_elems * kRing * 4))) return rc;
            HIPCHECK(e, hipMemsetAsync(S.pinP[i].p, 0, (size_t)S.pslot_elems * kRing * 16, st));  // every slot: zero history wherever the ring starts
            if ((rc = dev_alloc(e, e->pre_stats[i], (size_t)B * 2 * (S.pre[i].grid_x + 1)))) return rc;
        }
        if ((rc = dev_alloc(e, S.preR, (size_t)B * T * e->F[0] * 8))) return rc;
    }
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j, Co = lvl == 0 ? 2 : e->Ch[lvl], Fi = e->F[lvl + 1];
        const size_t nR = lvl == 0 ? (size_t)B * T * Fi * 8 : (size_t)B * ((Co + 7) / 8) * T * 2 * Fi * 8;
        if ((rc = dev_alloc(e, S.decR[j], nR))) return rc;
        HIPCHECK(e, hipMemsetAsync(S.decR[j].p, 0, nR * sizeof(float), st));
        if (lvl > 0 && (rc = dev_alloc(e, S.decP[j], (size_t)B * ((Co + 7) / 8) * PL * T * e->F[lvl] * 4))) return rc;
    }
    return alloc_stats_p(e);
}

// The fused front end (io_fused.hip.h: k_stft_feat): STFT of the segment at `off` of every stream's microphones -> the feature octets in
// ring slot `cur` (pinP[0] where the pre-conv blocks run on the plane path, xinP[0] otherwise) and microphone 0's spectrum -> spec0 [b][t][f].
// Writes the ring slot, so it runs where k_featurize_p would: on the encoder's stream, after the slot's last reader.
bool stft_feat_route(const se_engine *e) { return e->io_fuse_on && (!e->variant || e->cp->pre_p); }

int stage_stft_feat_p(se_engine *e, int cur, const float *src, long strideB, long strideM, long off, long Lsrc, SigRows rows, cf2 *spec0, hipStream_t st) {
    se_convp_state &S = *e->cp;
    const int T = e->T, PL = operand_planes(e->precision), TF = T * e->F[0];
    uint4 *feat = e->variant ? reinterpret_cast<uint4 *>(S.pinP[0].p) + (long)cur * S.pslot_elems
                             : reinterpret_cast<uint4 *>(S.xinP[0].p) + (long)cur * S.slot_elems[0];
    ProfScope ps(e, "k_stft_feat", "stft_feat", 0, st);
    HIPCHECK(e, sig_stft_feat(e->sig, src, strideB, strideM, e->M, off, Lsrc, rows, e->Bact, spec0, (long)TF, e->F[0], 1, feat, (long)PL * TF, PL,
                              e->atan2_phase, st));
    return 0;
}

// The two convolution launches that the stages and the feature taps (read_tap_impl) share.  y / yp: the output in the plan's layout;
// stats: the slab of the norm that follows (nullptr: no statistics); act_on = false stores the pre-activation values, what a tap reads.
//
// Encoder level i on ring slots cur / prev (the conv time buffer) with `pl`: the level's own plan, or its R-layout twin (tap_enc_plan)
int launch_enc_conv_p(se_engine *e, int i, const ConvPPlan &pl, int cur, int prev, float *y, uint4 *yp, float *stats, bool act_on, hipStream_t st,
                      const char *label) {
    se_convp_state &S = *e->cp;
    ConvPArgs a = pl.a;
    a.xbase = reinterpret_cast<const uint4 *>(S.xinP[i].p);
    a.xbytes = (unsigned)((size_t)S.slot_elems[i] * kRing * 16);
    a.cur_off = (long)cur * S.slot_elems[i];
    a.prev_off = (long)prev * S.slot_elems[i];
    a.y = y; a.yp = yp;
    if (stats) { a.stats = stats; a.stats_nslot = pl.grid_x; a.stats_slot0 = 0; }
    if (!act_on) a.relu_lo = a.relu_hi = 0;
    return launch_conv_p(e, pl, a, st, label);
}

// The transposed convolution of decoder level j on the planes `xin` ([b][Ci8][planes][T][Fi]: decinP, or decP[j - 1]) -> y (R layout,
// parity-planar above the last level), in the form select_all_p chose for this batch: the pair launch, or one launch per parity; the
// merged four-row plan at the last level.  label: one name for every launch (a tap's); nullptr: the stage's per-launch names
int launch_dec_conv_p(se_engine *e, int j, const uint4 *xin, float *y, float *stats, bool act_on, hipStream_t st, const char *label = nullptr) {
    const int lvl = e->L - 1 - j;
    PLevel &pv = e->cp->pv[j];
    const int ne = pv.dec_even.grid_x, no = dec_odd_slots(pv);
    const size_t xin_bytes = (size_t)e->B * ((e->Ch[lvl + 1] + 7) / 8) * act_planes(e, PlaneBuf::kConvAct) * e->T * e->F[lvl + 1] * 16;
    int rc;
    for (ConvPPlan *q : {&pv.dec_even, &pv.dec_odd}) {
        if (!q->active || (q == &pv.dec_odd && pv.dec_pair_on)) continue;
        ConvPArgs a = q->a;
        if (!pv.dec_pair_on) a.ntap2 = 0;
        a.xbase = xin; a.xbytes = (unsigned)xin_bytes; a.cur_off = 0; a.prev_off = -1;
        a.y = y;
        a.stats = stats; a.stats_nslot = ne + no; a.stats_slot0 = q == &pv.dec_odd ? ne : 0; a.stats_slot02 = ne;
        if (!act_on) a.relu_lo = a.relu_hi = 0;
        const char *sfx = a.ntap2 ? "" : (q == &pv.dec_odd ? "_odd" : "_even");
        if ((rc = launch_conv_p(e, *q, a, st, label ? label : ("dec" + std::to_string(j) + sfx).c_str()))) return rc;
    }
    return 0;
}

// Stage 1 (plane path): features + encoder -> xinP[*][cur], gru_in[cur] (fp32, the bottleneck GEMM's A operand)
// feat_done: stage_stft_feat_p has already written the slot's features (spec is then not read)
int stage_encoder_p(se_engine *e, int cur, int prev, const cf2 *spec, long sB, long sM, long sT, long sF, hipStream_t st, bool feat_done = false) {
    se_convp_state &S = *e->cp;
    const int L = e->L, T = e->T, B = e->B, PL = operand_planes(e->precision);
    const int Ba = e->Bact;  // launch batch: the prefix of streams that take part in this segment (se_realtime_process_ragged), B otherwise
    int rc;
    if (e->variant && S.pre_p) {  // features and the three pre-conv blocks x = m(x) + x on the plane path
        const int TF = T * e->F[0], C0 = e->Ch[0];
        if (!feat_done) {
            ProfScope ps(e, "k_featurize_p", "featurize", 0, st);
            FeatPArgs f{spec, sB, sM, sT, sF, reinterpret_cast<uint4 *>(S.pinP[0].p) + (long)cur * S.pslot_elems, (long)PL * TF, e->M, T, e->F[0], e->atan2_phase};
            launch_k_featurize_p(PL, dim3((TF + 255) / 256, Ba), st, f);
            HIPCHECK(e, hipGetLastError());
        }
        for (int i = 0; i < e->npre; i++) {
            ConvPPlan &pl = S.pre[i];
            ConvPArgs a = pl.a;
            a.xbase = reinterpret_cast<const uint4 *>(S.pinP[i].p);
            a.xbytes = (unsigned)((size_t)S.pslot_elems * kRing * 16);
            a.cur_off = (long)cur * S.pslot_elems;
            a.prev_off = (long)prev * S.pslot_elems;
            a.y = S.preR.p;
            a.stats = e->pre_stats[i].p; a.stats_nslot = pl.grid_x; a.stats_slot0 = 0;
            if ((rc = slab_fits(e, e->pre_stats[i], pl.grid_x, "a pre-conv block"))) return rc;
            if ((rc = launch_conv_p(e, pl, a, st, ("pre" + std::to_string(i)).c_str()))) return rc;
            ProfScope ps(e, "k_gln_p", "gln", 0, st);
            GlnPArgs g{};
            g.x = S.preR.p; g.x_stream = a.y_stream; g.C = C0; g.C8 = 1; g.T = T; g.F = e->F[0]; g.in_oT = e->F[0];
            g.w = e->lv[i].pre_nw.p; g.b = e->lv[i].pre_nb.p;
            g.st = SlabStats{e->pre_stats[i].p, pl.grid_x, (long)C0 * TF, e->eps_mode};
            g.res = reinterpret_cast<const uint4 *>(S.pinP[i].p) + (long)cur * S.pslot_elems; g.res_stream = (long)PL * TF;
            g.mode = 0;
            g.y = i + 1 < e->npre ? reinterpret_cast<uint4 *>(S.pinP[i + 1].p) + (long)cur * S.pslot_elems
                                  : reinterpret_cast<uint4 *>(S.xinP[0].p) + (long)cur * S.slot_elems[0];
            g.y_stream = (long)PL * TF;
            launch_k_gln_p(PL, dim3((TF + 1023) / 1024, 1, Ba), st, g);
            HIPCHECK(e, hipGetLastError());
        }
    } else if (e->variant) {  // the same blocks on their fp32 vector-ALU kernel (stage_features_pre), then one conversion into the P layout
        if ((rc = stage_features_pre(e, cur, spec, sB, sM, sT, sF, st))) return rc;
        ProfScope ps(e, "k_f32_to_p", "feat_to_p", 0, st);
        const int TF = T * e->F[0];
        F32ToPArgs f{e->pre_out.p, reinterpret_cast<uint4 *>(S.xinP[0].p) + (long)cur * S.slot_elems[0], (long)PL * TF, e->Ch[0], TF};
        launch_k_f32_to_p(PL, dim3((TF + 255) / 256, Ba), st, f);
        HIPCHECK(e, hipGetLastError());
    } else if (!feat_done) {
        ProfScope ps(e, "k_featurize_p", "featurize", 0, st);
        const int TF = T * e->F[0];
        FeatPArgs f{spec, sB, sM, sT, sF, reinterpret_cast<uint4 *>(S.xinP[0].p) + (long)cur * S.slot_elems[0], (long)PL * TF, e->M, T, e->F[0], e->atan2_phase};
        launch_k_featurize_p(PL, dim3((TF + 255) / 256, Ba), st, f);
        HIPCHECK(e, hipGetLastError());
    }
    for (int i = 0; i < L; i++) {
        const int Co = e->Ch[i + 1], Fo = e->F[i + 1];
        ConvPPlan &pl = S.pv[i].enc;
        const ConvPArgs &a = pl.a;
        int nslot = pl.grid_x;
        if (e->variant) nslot = S.pv[i].gate[0].grid_x + (S.pv[i].gate[1].active ? S.pv[i].gate[1].grid_x : 0);
        if ((rc = slab_fits(e, e->enc_stats[i], nslot, "an encoder level"))) return rc;
        if (!e->variant) {
            if ((rc = launch_enc_conv_p(e, i, pl, cur, prev, S.encR[i].p, nullptr, e->enc_stats[i].p, true, st, ("enc" + std::to_string(i)).c_str()))) return rc;
        } else {
            if ((rc = launch_enc_conv_p(e, i, pl, cur, prev, nullptr, reinterpret_cast<uint4 *>(S.encA[i].p), nullptr, true, st, ("enc" + std::to_string(i)).c_str()))) return rc;
            const int n0 = S.pv[i].gate[0].grid_x, n1 = S.pv[i].gate[1].active ? S.pv[i].gate[1].grid_x : 0;
            nslot = n0 + n1;
            for (int part = 0; part < 2; part++) {
                ConvPPlan &gp = S.pv[i].gate[part];
                if (!gp.active) continue;
                ConvPArgs g = gp.a;
                g.xbase = reinterpret_cast<const uint4 *>(S.encA[i].p);
                g.xbytes = (unsigned)((size_t)B * ((Co + 7) / 8) * PL * T * Fo * 16);
                g.cur_off = 0; g.prev_off = -1;
                g.y = S.encR[i].p;
                g.stats = e->enc_stats[i].p; g.stats_nslot = nslot; g.stats_slot0 = part ? n0 : 0;
                if ((rc = launch_conv_p(e, gp, g, st, ("gate" + std::to_string(i)).c_str()))) return rc;
            }
        }
        ProfScope ps(e, "k_gln_p", "gln", 0, st);
        GlnPArgs g{};
        g.x = S.encR[i].p; g.x_stream = a.y_stream; g.C = Co; g.C8 = (Co + 7) / 8; g.T = T; g.F = Fo; g.in_oT = Fo;
        g.w = e->lv[i].enc_nw.p; g.b = e->lv[i].enc_nb.p;
        g.st = SlabStats{e->enc_stats[i].p, nslot, (long)Co * T * Fo, e->eps_mode};
        if (i + 1 < L) {
            g.mode = 0;
            g.y = reinterpret_cast<uint4 *>(S.xinP[i + 1].p) + (long)cur * S.slot_elems[i + 1];
            g.y_stream = (long)g.C8 * act_planes(e, PlaneBuf::kConvAct) * T * Fo;
            launch_k_gln_p(PL, dim3((T * Fo + 1023) / 1024, g.C8, Ba), st, g, act_format(e, PlaneBuf::kConvAct));
        } else if (e->gemm_p) {  // last level = A operand of the GRU input projection, as split-bf16 planes (k_gemm_p)
            g.mode = kblock_on(e) ? 2 : 1;  // (2: the same operand K-blocked, gemm_kblock.h)
            g.y = reinterpret_cast<uint4 *>(e->gruinP[cur].p);
            g.y_plane = (long)B * T * g.C8 * Fo;
            launch_k_gln_p(PL, dim3((T * Fo + 1023) / 1024, g.C8, Ba), st, g, buffer_format(e->precision, e->pair_on, PlaneBuf::kGemmA));
        } else {  // last level feeds the fp32 GEMM of the bottleneck (launch_gemm): [T][C*F] rows
            GlnEwArgs ge{nullptr, e->gru_in[cur].p, g.w, g.b, g.st, 3, Co, T, Fo, nullptr};
            ge.x = S.encR[i].p;
            const long n = (long)Co * T * Fo;
            hipLaunchKernelGGL(k_gln_r2t, dim3((unsigned)((n / 8 + 255) / 256), B), dim3(256), 0, st, ge, a.y_stream);
        }
        HIPCHECK(e, hipGetLastError());
    }
    return 0;
}

// Stage 3 (plane path): decoder + mask.  The bottleneck's k_gln2_p has already written decinP[cur].
// wav (optional): the fused back end (io_fused.hip.h: k_mask_istft) takes the place of k_final_mask_p and writes stream b's K samples to
// wav + b * wav_ld; `out` is then not written.
int stage_decoder_p(se_engine *e, int cur, const cf2 *spec, long sB, long sT, long sF, cf2 *out, long oB, long oT, long oF, hipStream_t st,
                    float *wav = nullptr, long wav_ld = 0) {
    se_convp_state &S = *e->cp;
    const int L = e->L, T = e->T, B = e->B, PL = operand_planes(e->precision);
    const int APL = act_planes(e, PlaneBuf::kConvAct);  // planes of decinP, decP and of the skip path's xinP[lvl >= 1]
    const int Ba = e->Bact;  // launch batch: the prefix of streams that take part in this segment (se_realtime_process_ragged), B otherwise
    int rc;
    const uint4 *xin = reinterpret_cast<const uint4 *>(S.decinP[cur].p);
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j;
        const int Co = lvl == 0 ? 2 : e->Ch[lvl], Fi = e->F[lvl + 1], Fo = 2 * Fi - 1;
        PLevel &pv = S.pv[j];
        const int ne = pv.dec_even.grid_x, no = dec_odd_slots(pv);
        if ((rc = slab_fits(e, e->dec_stats[j], ne + no, "a decoder level"))) return rc;
        if ((rc = launch_dec_conv_p(e, j, xin, S.decR[j].p, e->dec_stats[j].p, true, st))) return rc;
        const SlabStats sy{e->dec_stats[j].p, ne + no, (long)Co * T * Fo, e->eps_mode};
        if (lvl > 0) {
            const int Fr = e->F[lvl];
            const long nu = (long)Co * T * Fr;
            const uint4 *res = reinterpret_cast<const uint4 *>(S.xinP[lvl].p);
            const unsigned res_bytes = (unsigned)((size_t)S.slot_elems[lvl] * kRing * 16);
            // one workgroup per stream: below ~100 streams most CUs would idle, the two k_conv_p launches (statistics, gate) spread
            // over positions instead (B = 1: 24 vs 45 us per level).  SE_SKIP_MIN_BATCH moves the crossover.
            if (pv.sk.active && B >= e->skip_min_batch) {
                SkipPArgs a = pv.sk.a;
                a.x = res + (long)cur * S.slot_elems[lvl];
                a.ydec = S.decR[j].p;
                a.sy = sy;
                a.out = reinterpret_cast<uint4 *>(S.decP[j].p);
                ProfScope ps(e, pv.sk_fmt == PlaneFmt::kF16Pair && pv.sk.wpl == kPairPlanesW2 ? "k_skip_p_w2" : "k_skip_p", ("skip" + std::to_string(j)).c_str(), pv.sk.flops * B, st);
                if (launch_k_skip_p(pv.sk.wpl, pv.sk.KP, Ba, pv.sk.lds, st, a, pv.sk_fmt, e->skip_depth)) return fail(e, SE_ERR_ARG, "no k_skip_p instance for %d planes x %d K steps", PL, pv.sk.KP);
                HIPCHECK(e, hipGetLastError());
            } else {
            {
                ConvPArgs a = pv.skipm.a;
                a.xbase = res; a.xbytes = res_bytes; a.cur_off = (long)cur * S.slot_elems[lvl]; a.prev_off = -1;
                a.y = nullptr; a.out_mode = kPOutStats;
                a.stats = e->skip_stats[j].p; a.stats_nslot = pv.skipm.grid_x; a.stats_slot0 = 0;
                if ((rc = slab_fits(e, e->skip_stats[j], pv.skipm.grid_x, "a skip gate"))) return rc;
                if ((rc = launch_conv_p(e, pv.skipm, a, st, ("skipstat" + std::to_string(j)).c_str()))) return rc;
            }
            {
                ConvPArgs a = pv.skip.a;
                a.xbase = res; a.xbytes = res_bytes; a.cur_off = (long)cur * S.slot_elems[lvl]; a.prev_off = -1;
                a.yp = reinterpret_cast<uint4 *>(S.decP[j].p);
                a.yp_stream = (long)((Co + 7) / 8) * APL * T * Fr;
                a.bl_ydec = S.decR[j].p; a.bl_stream = pv.dec_even.a.y_stream; a.bl_oT = 2 * Fi; a.bl_Fh = Fi; a.bl_Fo = Fo;
                a.bl_nw = e->lv[j].dec_nw.p; a.bl_nb = e->lv[j].dec_nb.p; a.bl_mnw = e->lv[j].dec_mnw.p; a.bl_mnb = e->lv[j].dec_mnb.p;
                a.bl_sy = sy; a.bl_su = SlabStats{e->skip_stats[j].p, pv.skipm.grid_x, nu, e->eps_mode};
                if ((rc = launch_conv_p(e, pv.skip, a, st, ("skip" + std::to_string(j)).c_str()))) return rc;
            }
            }
            xin = reinterpret_cast<const uint4 *>(S.decP[j].p);
        } else {
            if (Fo != e->F[0]) return fail(e, SE_ERR_ARG, "decoder output has %d bins, spectrum has %d", Fo, e->F[0]);
            MaskPArgs m{S.decR[j].p, (long)T * Fi * 8, Fi, e->lv[j].dec_nw.p, e->lv[j].dec_nb.p, sy, spec, sB, sT, sF, out, oB, oT, oF, T, e->F[0]};
            if (wav) {
                ProfScope ps(e, "k_mask_istft", "mask_istft", 0, st);
                HIPCHECK(e, sig_mask_istft(e->sig, m, Ba, wav, wav_ld, st));
            } else {
                ProfScope ps(e, "k_final_mask_p", "final_mask", 0, st);
                launch_k_final_mask_p(dim3((T * e->F[0] + 1023) / 1024, Ba), st, m);
                HIPCHECK(e, hipGetLastError());
            }
        }
    }
    return 0;
}

// P layout (device) -> reference layout [B][C][F][T] on the host (debug taps / state export); fp32 = sum of the planes
// fmt: the format of the buffer `dev` points into (the fp16 pair is joined as the device readers join it: join2h)
int p_to_host(se_engine *e, const float *dev, PlaneFmt fmt, int C, int F, float *host_out, hipStream_t st, bool to_bcft) {
    const bool pair = fmt == PlaneFmt::kF16Pair;
    const int T = e->T, B = e->B, PL = pair ? kPairPlanesA : operand_planes(e->precision), C8 = (C + 7) / 8;
    const size_t n16 = (size_t)B * C8 * PL * T * F;  // uint4 count
    std::vector<uint16_t> h(n16 * 8);
    HIPCHECK(e, hipStreamSynchronize(st));
    HIPCHECK(e, hipMemcpy(h.data(), dev, n16 * 16, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++)
        for (int c = 0; c < C; c++)
            for (int t = 0; t < T; t++)
                for (int f = 0; f < F; f++) {
                    float v = 0;
                    uint16_t up[3] = {0, 0, 0};
                    for (int pl = 0; pl < PL; pl++) {
                        const uint16_t u = h[(((((size_t)b * C8 + c / 8) * PL + pl) * T + t) * F + f) * 8 + c % 8];
                        up[pl] = u;
                        if (pair) continue;
                        if (PL == 1) { _Float16 hv; memcpy(&hv, &u, 2); v += (float)hv; }
                        else v += bf16_to_f32(u);
                    }
                    if (pair) v = join2h(up[0], up[1]);
                    if (to_bcft) host_out[(((size_t)b * C + c) * F + f) * T + t] = v;
                    else host_out[(((size_t)b * C + c) * T + t) * F + f] = v;
                }
    return SE_OK;
}

int host_to_p(se_engine *e, const std::vector<float> &src, PlaneFmt fmt, int C, int F, float *dev);

// A weight load that changes the format of the convolution path's buffers (the range guard, once per load) between two calls of a
// running batch: the conv history in the current ring slot of xinP[i >= 1] is re-written in the new format, through the host.  Every
// other plane buffer is written before it is read within a segment.
int convert_history_p(se_engine *e) {
    se_convp_state &S = *e->cp;
    const PlaneFmt now = act_format(e, PlaneBuf::kConvAct);
    if (e->B <= 0 || !S.xinP[0].p || S.ring_fmt == now) { S.ring_fmt = now; return 0; }
    HIPCHECK(e, hipDeviceSynchronize());
    for (int i = 1; i < e->L; i++) {
        std::vector<float> h((size_t)e->B * e->Ch[i] * e->T * e->F[i]);
        float *slot = S.xinP[i].p + (size_t)e->slot * S.slot_elems[i] * 4;
        int rc = p_to_host(e, slot, S.ring_fmt, e->Ch[i], e->F[i], h.data(), nullptr, false);
        if (!rc) rc = host_to_p(e, h, now, e->Ch[i], e->F[i], slot);
        if (rc) return rc;
    }
    S.ring_fmt = now;
    return 0;
}

// host [B][C][T][F] fp32 -> P layout on the device (state import)
int p_to_host(se_engine *e, const float *dev, PlaneBuf kind, int C, int F, float *host_out, hipStream_t st, bool to_bcft) {
    return p_to_host(e, dev, act_format(e, kind), C, F, host_out, st, to_bcft);
}

int host_to_p(se_engine *e, const std::vector<float> &src, PlaneFmt fmt, int C, int F, float *dev) {
    const bool pair = fmt == PlaneFmt::kF16Pair;
    const int T = e->T, B = e->B, PL = pair ? kPairPlanesA : operand_planes(e->precision), C8 = (C + 7) / 8;
    std::vector<uint16_t> h((size_t)B * C8 * PL * T * F * 8, 0);
    for (int b = 0; b < B; b++)
        for (int c = 0; c < C; c++)
            for (int t = 0; t < T; t++)
                for (int f = 0; f < F; f++) {
                    const float x = src[(((size_t)b * C + c) * T + t) * F + f];
                    uint16_t parts[3];
                    if (pair) split2h(x, parts[0], parts[1]);
                    else if (PL == 1) parts[0] = f16_rne(x);
                    else {
                        parts[0] = bf16_rne(x);
                        const float r1 = x - bf16_to_f32(parts[0]);
                        parts[1] = bf16_rne(r1);
                        parts[2] = bf16_rne(r1 - bf16_to_f32(parts[1]));
                    }
                    for (int pl = 0; pl < PL; pl++) h[(((((size_t)b * C8 + c / 8) * PL + pl) * T + t) * F + f) * 8 + c % 8] = parts[pl];
                }
    HIPCHECK(e, hipMemcpy(dev, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    return SE_OK;
}

int host_to_p(se_engine *e, const std::vector<float> &src, PlaneBuf kind, int C, int F, float *dev) {
    return host_to_p(e, src, act_format(e, kind), C, F, dev);
}

}  // namespace
