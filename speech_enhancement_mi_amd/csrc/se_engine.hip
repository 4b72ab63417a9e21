// se_engine.hip - persistent stream-batch engine behind the C ABI of include/se_engine.h.
//
// One engine owns, on one MI355X: all weights (re-laid-out once for the kernels), all per-stream
// state for B streams (ring slots of activation tensors that double as the reference's conv time buffers,
// GRU hidden state) and a fixed kernel sequence that advances every stream by one K-sample window:
//
//   k_stft -> [CRN_ELU / student: 3x pre-conv block] -> encoder and decoder on the plane path (convp_engine.inc.h:
//   k_conv_p, k_gln_p, k_skip_p, k_final_mask_p) around the bottleneck (GEMMs + T x k_gru_step per layer) -> k_istft
//
// In se_step / se_realtime_process the two ends run fused (io_fused.hip.h): k_stft_feat = k_stft + k_featurize_p where the features
// go to the plane path, k_mask_istft = k_final_mask_p + k_istft; SE_IO_FUSE=0 keeps the four kernels.
//
// k_conv_small / k_preconv_tb (plan_conv, launch_conv) run the fp32 / bf16x3 pre-conv blocks, k_conv_igemm the training path;
// k_gemm_x / k_gemm_tn are the bottleneck GEMMs where the plane GEMM k_gemm_p does not apply.  The student's feature taps re-run
// the plane path's own launches (read_tap_impl).  Reference: TemporalCRN.forward / realtime_process (CRN.py:454-496, 560-589).
// No CPU fallback exists: every entry point fails with SE_ERR_HIP if the device path is unavailable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/se_engine.h"
#include "conv_dispatch.h"
#include "convp_dispatch.h"
#include "fsn.hip.h"
#include "fft_lds.h"
#include "gemm.hip.h"
#include "gru_pack.h"
#include "norm.hip.h"
#include "stft.hip.h"
#include "state_rows.hip.h"
#include "chain_plan.h"
#include "engine_host.h"
#include "sig_chain.h"

using namespace se;

namespace {

constexpr int kFftSub = 8;      // segments per STFT / iSTFT launch inside the pipelined path
constexpr int kPipeChunk = 64;  // segments per pipelined chunk (bounds spec_all / mask_all)
constexpr int kRing = 4;  // stage-crossing activation slots (see se_engine::slot)

struct ConvPlan {  // one launch of the vector-ALU convolution (k_conv_small / k_preconv_tb)
    ConvArgs a{};  // pointers filled per launch
    int grid_x = 0;
    size_t lds = 0;
    DevBuf w, bias;
    bool active = false;
    DevBuf gatew;     // fused gated 1x1 pair weights
    double flops = 0;  // algorithmic FLOPs per stream per launch (SURVEY.md 8d accounting)
};

struct Level {  // one encoder/decoder level: the norm affines, and the pre-conv block that shares the index
    ConvPlan pre;          // CRN_ELU preconv block i (levels 0..2): 5x5 frequency-dilated conv with the gated pair fused in
    DevBuf enc_nw, enc_nb, dec_nw, dec_nb, dec_mnw, dec_mnb, pre_nw, pre_nb;
};

}  // namespace

struct se_engine : EngineHost {
    se_config c{};
    int L = 0, T = 0, D = 0, M = 0, K = 0, N = 0, H = 0, NL = 0;
    int F[SE_MAX_LEVELS + 1]{};
    int Ch[SE_MAX_LEVELS + 1]{};  // Ch[0] = 2M-1, Ch[i+1] = channels[i]
    bool weights_ready = false;
    int gru_direct = -1;      // SE_GRU_DIRECT: 1 = always k_gru_step (W_hh streamed from L2), 0 = always k_gru_step2 (LDS slice),
                              // default -1 = k_gru_step in the overlapped (pipelined) bottleneck stage, k_gru_step2 otherwise
    int gru_split = -1;       // SE_GRU_SPLIT: the split-bf16 step kernel (k_gru_step_split) where eligible (gru_split_eligible): 1 = everywhere,
                              // 0 = never, default -1 = in the overlapped stage, and only while SE_GRU_DIRECT is unset

    SigChain sig;  // STFT / iSTFT tables and plan (sig_chain.h)

    // weights
    Level lv[SE_MAX_LEVELS];  // enc i at lv[i]; decoder j at lv[j] (dec_* members)
    DevBuf wih[4], whh[4], bih[4], bhh[4], fcw, fcb, gnw, gnb;
    DevBuf wih_x[4], fcw_x;  // bf16x3 planes [3][N][K] of the GEMM weights (k_gemm_bf16x6)
    DevBuf whh_p[4];         // W_hh as packed plane fragments (gru_pack.h; bf16, or the fp16 pair's when pair_on) for k_gru_step_split:
                             // precision 0 and H % 32 == 0 only
    int variant = 0, act = 1, eps_mode = 0, atan2_phase = 0, npre = 0;  // derived from se_config.variant
    int precision = 0;        // se_config.precision: 0 = bf16x6 (3 operand planes), 1 = fp16 operands (1 plane), 2 = bf16x3 (2 planes)
    int num_cu = 256;         // compute units of the device (MI355X: 256)

    // state + activations for B streams
    int B = 0;
    int parity = 0;  // index of the "current" half of the encoder-private ping-pong buffers (pin)
    // Buffers that cross the three stages of a segment (encoder -> recurrent bottleneck -> decoder) live in a ring of
    // kRing slots, so that in se_realtime_process the encoder of segment n+1.. can run on its own HIP stream while the
    // latency-bound GRU recurrence of segment n and the decoder of segment n-1 are still in flight.  slot = segment % kRing.
    // The plane path's activation rings are in se_convp_state; the fp32 tensors here are the output of the vector-ALU pre-conv
    // blocks (pre_out) and the fp32 GRU input (gru_in).
    int slot = 0;
    DevBuf spec[kRing], maskspec;
    DevBuf spec_all, mask_all;         // pipelined se_realtime_process: spectra / masked spectra of one chunk of segments
    DevBuf gru_in[kRing], gi0[kRing], gil[4], seqr[4][kRing], hbuf[4][2], fc_out;  // gi0 / seqr cross stage streams: rings
    int pipeline = 1;                  // SE_PIPELINE=0: one stream, stages back to back
    hipStream_t stage_stream[3]{};      // encoder (+ GRU input projection) / decoder (fc + norm first) / recurrence (all layers)
    hipEvent_t ev_enc[kRing]{}, ev_gru[kRing]{}, ev_dec[kRing]{}, ev_fork{}, ev_join{};
    bool stage_ready = false;
    int hcur[4]{};
    DevBuf enc_stats[SE_MAX_LEVELS], dec_stats[SE_MAX_LEVELS], skip_stats[SE_MAX_LEVELS];  // [B][slots][2] norm partials
    DevBuf pin[3][2], pre_g, pre_stats[3];  // CRN_ELU preconv chain (inputs ping-ponged: they carry 4 history columns)
    DevBuf pre_out;                         // its fp32 output (written and converted to planes on one stream: no ring)
    DevBuf yseg;
    // A ragged / chains call is described by its ChainPlan (chain_plan.h), which run_segments gets as an argument.  What the engine keeps:
    // plan_dev, the device copy of the plan's per-stream vectors (8 * B floats); carry_*, one row per stream in the live tensors' row
    // layout (state_rows_of), filled when a stream's last segment has passed the stage that owns the tensor, written back at call exit.
    DevBuf plan_dev, carry_x[SE_MAX_LEVELS], carry_p[3], carry_h[4];
    // Prefix compaction: every layout is stream-major, so when the plan is `compact` the streams that still take part in segment n are a
    // PREFIX of the batch and every launch of that segment simply covers Bact = plan->bact(n) < B streams (grids, GEMM rows, GRU rows);
    // strides and plane sizes stay those of the allocation batch B.  Bact is set per stage call by run_segments.
    int Bact = 0;
    int bact_slot[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // launch batch of the segment living in each ring slot (the lagged GRU rounds mix segments)
    // plane-layout convolution path (conv_p.hip.h, convp_engine.inc.h): activations as split-bf16 planes
    struct se_convp_state *cp = nullptr;
    // plane-layout bottleneck GEMMs (k_gemm_p): A operands arrive as split-bf16 planes from their producers
    bool gemm_p = false;      // decided in ensure_ready: K dimensions multiples of 32 (SE_GEMM_P=0 disables);
                              // off for batches of <= 64 GEMM rows (se_reset), which run on the skinny fp32 kernel instead
    bool gemm_p_cap = false;
    // measured crossovers (profiles: B = 16 / 32 / 64 / 128, 512-pt): the skinny kernel wins up to 640 GEMM rows (B = 32:
    // 133 vs 228 us for the three GEMMs) and ties at 1280; the two-launch skip gate wins up to B = 64 (119 vs 147 us)
    int skinny_rows = 800;    // SE_GEMM_SKINNY_ROWS: bottleneck GEMMs with up to this many rows run on the skinny fp32 kernel
    int skip_min_batch = 96;  // SE_SKIP_MIN_BATCH: the streaming skip kernel needs at least this many streams
    int skip_depth = -1;      // SE_SKIP_DEPTH: tiles per batch of the streaming skip kernel (k_skip_pd); 0: k_skip_p; -1: per instance (se_skip.hip)
    int dec_pair = 1;         // SE_DEC_PAIR=0: the transposed convolutions above the last level run one k_conv_p launch per parity
    int dec_pair_site[SE_MAX_LEVELS];  // SE_DEC_PAIR_dec<j> = 0 / 1: decoder level j on two launches / on the pair launch, whatever the cost model says; -1: the model
    int io_fuse = 1;          // SE_IO_FUSE=0: k_stft + k_featurize_p and k_final_mask_p + k_istft as four kernels (io_fused.hip.h fuses them)
    bool io_fuse_on = false;  // io_fuse and the fused kernels' workgroups fit a CU's LDS at this geometry
    int gemm_p_env = 1;
    DevBuf gruinP[kRing], seqP[4][kRing];  // [PL][B*T][D'] / [PL][B*T][H] planes (PlaneBuf::kGemmA: bf16, or two fp16 planes when pair_on)
    DevBuf wih_xp;                          // W_ih0 planes with K in the engine's feature order (k_gemm_p)
    // fp16 pair format (split_f16pair.h) on the bottleneck: gruinP / seqP as two fp16 planes, the k_gemm_p weights (wih_xp, wih_h,
    // fcw_xp) and whh_p as (2^11 hi, lo, hi), three MFMA terms instead of six
    int f16_pair = 1;         // SE_F16_PAIR=0: the bf16 route (three planes, six terms) everywhere
    int f16_pair_conv = 1;    // SE_F16_PAIR_CONV=0: the pair on the bottleneck only; xinP[i >= 1], decinP, decP and their kernels on bf16 planes
    bool pair_on = false;     // decided once per weight load (f16_pair_decide): knob, eligibility and the range guard
    int pair_w3 = 0;          // SE_PAIR_W3=1: pair weights as the three stored planes (2^11 hi, lo, hi) and the kernels' three-plane instances;
                              // default: two stored planes (lo, hi), 2^11 hi made in registers - the same bits from fewer weight bytes
    int gemm_kblock = 1;      // SE_GEMM_KBLOCK=0: gruinP / seqP and the k_gemm_p weights stay plane-major where they would be K-blocked (kblock_on)
    DevBuf wih_h[4];          // W_ih of layers >= 1 as pair planes (wih_x[l] stays bf16: the fp32-row GEMMs of small batches read it)
    // fc_output_layer + gLN(last) on the plane GEMM route: weight rows, bias and the norm's per-element affine permuted like W_ih0's
    // K axis, so that fc_out column (o * F + f) * 8 + c holds reference feature (8 o + c) * F + f (channels padded to whole octets
    // with zero rows); fc_stats [B][T * column tiles][2] = per-row (sum, sum of squares) partials from the GEMM's epilogue
    DevBuf fcw_xp, fcb_p, gnw_p, gnb_p, fc_stats;
    int dbg_skip = 0;         // SE_DBG_SKIP bit mask, TIMING EXPERIMENTS ONLY (results are wrong): 1 = no GRU step launches, 2 = no bottleneck
                              // GEMMs, 4 = no encoder convolutions, 8 = no decoder

    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline leg)
    bool prof_on = false;
    struct ProfRec { int label; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    struct ProfLabel { std::string kernel, label; double flops; double ms = 0; long launches = 0; };
    std::vector<ProfLabel> prof_labels;
};

namespace {

// format / plane count of an activation plane buffer of this engine (engine_host.h: buffer_format); encoder level i reads xinP[i]
PlaneFmt act_format(const se_engine *e, PlaneBuf kind) { return buffer_format(e->precision, e->pair_on, kind, e->f16_pair_conv != 0); }
int act_planes(const se_engine *e, PlaneBuf kind) { return buffer_planes(e->precision, e->pair_on, kind, e->f16_pair_conv != 0); }
PlaneBuf xin_kind(int level) { return level == 0 ? PlaneBuf::kFeature : PlaneBuf::kConvAct; }
// stored planes of a weight in the fp16 pair format (split_f16pair.h)
int pair_wplanes(const se_engine *e) { return e->pair_w3 ? kPairPlanesW : kPairPlanesW2; }
// gruinP, seqP and the weights k_gemm_p multiplies them with are K-blocked (engine_host.h: buffer_kblocked, gemm_kblock.h).  Like pair_on it
// is fixed per weight load; the buffers' sizes do not depend on it
bool kblock_on(const se_engine *e) { return buffer_kblocked(e->precision, e->pair_on, pair_wplanes(e), e->gemm_kblock != 0, PlaneBuf::kGemmA); }

int prof_label(se_engine *e, const char *kernel, const std::string &label, double flops) {
    for (size_t i = 0; i < e->prof_labels.size(); i++)
        if (e->prof_labels[i].label == label) { e->prof_labels[i].flops = flops; return (int)i; }
    e->prof_labels.push_back({kernel, label, flops});
    return (int)e->prof_labels.size() - 1;
}

struct ProfScope {  // brackets one launch with two events when profiling is on
    se_engine *e;
    hipStream_t st;
    int idx = -1;
    ProfScope(se_engine *e_, const char *kernel, const std::string &label, double flops, hipStream_t st_) : e(e_), st(st_) {
        if (!e->prof_on) return;
        hipEvent_t ev[2];
        for (auto &x : ev) {
            if (!e->prof_pool.empty()) { x = e->prof_pool.back(); e->prof_pool.pop_back(); }
            else if (hipEventCreate(&x) != hipSuccess) return;
        }
        e->prof_recs.push_back({prof_label(e, kernel, label, flops), ev[0], ev[1]});
        idx = (int)e->prof_recs.size() - 1;
        (void)hipEventRecord(ev[0], st);
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(e->prof_recs[idx].b, st);
    }
};

std::string canon(const char *key) {
    std::string k(key);
    size_t pos = k.find(".net.0.");
    if (pos != std::string::npos) k.replace(pos, 7, ".conv.");  // CRN.py:314-316 alias
    return k;
}

// ---- conv planning --------------------------------------------------------------------------------
// The vector-ALU convolution of the pre-conv blocks (up to 8 channels, crn_geometry_supported): one thread per position, direct
// global reads, weights [tap][ci][CW] in LDS.
// taps: list of (kf, kt) with their patch offsets; wsel(ci, co, kf, kt) fetches the reference weight.
template <class WSel>
int plan_conv(se_engine *e, ConvPlan &pl, int Ci, int Co, int FP, int Fi, int Fy, int s, int os, int oo, int colpad,
              int tlo_off, int ngroup, int dil, int St, const std::vector<std::array<int, 4>> &taps /*kf,kt,rowgrp,coloff*/,
              WSel wsel, const std::vector<float> &bias, int relu_lo, int relu_hi, int act) {
    pl.active = FP > 0;
    if (!pl.active) return 0;
    if (Co > 8) return fail(e, SE_ERR_ARG, "the vector-ALU convolution supports up to 8 output channels, got %d", Co);
    const int T = e->T;
    const int ntap = (int)taps.size();
    const int P = T * FP;
    const int CW = Co <= 4 ? 4 : 8;
    ConvArgs &a = pl.a;
    a.par_rows = 0;
    a.Ci = Ci; a.Co = Co; a.CoPad = CW; a.T = T; a.Fi = Fi; a.FP = FP; a.Fy = Fy;
    a.s = s; a.os = os; a.oo = oo; a.colpad = colpad; a.tlo_off = tlo_off; a.ngroup = ngroup; a.dil = dil; a.grouped = 0;
    a.ntap = ntap; a.CC = Ci; a.nchunk = 1; a.tiles_per_wg = 8; a.St = St;
    a.relu_lo = relu_lo; a.relu_hi = relu_hi; a.act = act; a.Cy = Co; a.cy0 = 0;
    for (int t = 0; t < ntap; t++) { a.rowgrp[t] = taps[t][2]; a.coloff[t] = taps[t][3]; }
    pl.grid_x = (P + 255) / 256;
    pl.lds = sizeof(float) * (size_t)ntap * Ci * CW;
    if (pl.lds > 64 * 1024) return fail(e, SE_ERR_ARG, "small-conv weights do not fit LDS");
    std::vector<float> w((size_t)ntap * Ci * CW, 0.0f);
    for (int t = 0; t < ntap; t++)
        for (int ci = 0; ci < Ci; ci++)
            for (int co = 0; co < Co; co++) w[((size_t)t * Ci + ci) * CW + co] = wsel(ci, co, taps[t][0], taps[t][1]);
    int rc = dev_upload(e, pl.w, w);
    if (rc) return rc;
    return dev_upload(e, pl.bias, bias);
}

// The CRN geometries the engine accepts, stated in one place and checked before any planning (se_reset and every other entry
// point that plans fails with SE_ERR_ARG and the message).  A convolution's output channels are GEMM rows in tiles of 32, of
// which a workgroup's four waves take 1, 2 or 4 (never 3).  Finer limits of the kernels' own tilings are reported by
// plan_conv / plan_conv_p from the same call.
bool crn_geometry_supported(const se_engine *e, std::string *why) {
    char msg[256];
    auto refuse = [&](const char *fmt, int a, int b) { snprintf(msg, sizeof(msg), fmt, a, b); *why = msg; return false; };
    auto rows_ok = [](int rows) { const int tiles = (rows + 31) / 32; return tiles <= 4 && tiles != 3; };
    if (e->Ch[0] > 128) return refuse("%d microphones give %d feature channels: at most 128 are supported (num_inputs <= 64)", e->M, e->Ch[0]);
    if (e->variant && e->Ch[0] > 8) return refuse("the pre-conv blocks support up to 8 feature channels (num_inputs <= 4), got %d inputs = %d channels", e->M, e->Ch[0]);
    for (int i = 0; i < e->L; i++) {
        const int C = e->Ch[i + 1];
        if (!rows_ok(C)) return refuse("encoder block %d has %d channels: up to 64 or 97-128 are supported (GEMM rows in 1, 2 or 4 tiles of 32)", i, C);
        // decoder skip connection (levels 1..L-1): residualmask / residual stacked as 2 C rows of one 1x1 GEMM
        if (i + 1 < e->L && !rows_ok(2 * C))
            return refuse("the skip connection of level %d has %d channels: its 1x1 pair needs 2 GEMM rows per channel, so up to 32 or 49-64 channels are supported", i + 1, C);
        // CRN_ELU / student: the gated 1x1 pair (conv_trans, conv_gated) as 2 rows per channel, in halves above 64 channels
        if (e->variant && !(C > 64 ? rows_ok(2 * ((C + 1) / 2)) && rows_ok(2 * (C / 2)) : rows_ok(2 * C)))
            return refuse("encoder block %d has %d channels: its gated 1x1 pair needs 2 GEMM rows per channel and up to 64 channels per launch; 33-48 channels per launch are not supported", i, C);
    }
    return true;
}

// whether the engine's shapes allow the plane GEMM route at all (which batches take it: select_gemm_route)
bool gemm_p_capable(const se_engine *e) { return e->gemm_p_env && e->D % 32 == 0 && e->H % 32 == 0 && e->Ch[e->L] % 8 == 0; }

// Range guard of the fp16 pair format, from the loaded parameters alone (never a run-time branch in a kernel): every activation that a
// norm writes into a plane buffer is bounded by max|gamma| sqrt(N) + max|beta| (N elements per stream: |x - mean| <= sqrt(N) sigma),
// the skip output of a decoder level by the larger of its two branches (pair_skip_bound: the decoder norm's bound, or the row L1 norm
// of residual.weight times the bound of `res`), and 2^11 w_hi must stay finite in fp16.  An activation bound above 6e4 or a weight
// operand of 2^4 or more keeps the whole engine on the bf16 route.  All norms and all weight operands are checked, also those whose buffers do not take the format yet, so the
// set of eligible checkpoints does not move when the convolution path follows.  (h_t is a convex combination of tanh values and
// h_{t-1}; a caller-supplied state beyond the fp16 range is clamped by split2h.)
bool f16_pair_guard(const se_engine *e) {
    auto absmax = [&](const std::string &key, float &m) {
        auto it = e->params.find(key);
        if (it == e->params.end()) return false;
        for (float v : it->second) {
            if (!(std::fabs(v) <= 3.0e38f)) return false;  // inf / NaN
            m = std::max(m, std::fabs(v));
        }
        return true;
    };
    auto norm_ok = [&](const std::string &prefix, double n, double *bound = nullptr) {
        float g = 0, b = 0;
        if (!absmax(prefix + "weight", g) || !absmax(prefix + "bias", b)) return false;
        const double bd = pair_norm_bound(g, b, n);
        if (bound) *bound = bd;
        return bd <= kPairGuardLimit;
    };
    const int L = e->L, T = e->T;
    double enc_bound[SE_MAX_LEVELS] = {};  // what convlist.i.norm writes: xinP[i + 1], the `res` of decoder level lvl = i + 1
    for (int i = 0; i < L; i++)
        if (!norm_ok("convlist." + std::to_string(i) + ".norm.", (double)e->Ch[i + 1] * T * e->F[i + 1], &enc_bound[i])) return false;
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j, Co = lvl == 0 ? 2 : e->Ch[lvl], Fo = 2 * e->F[lvl + 1] - 1;
        double dec_bound = 0;
        if (!norm_ok("deconvlist." + std::to_string(j) + ".norm.", (double)Co * T * Fo, &dec_bound)) return false;
        if (lvl > 0 && !norm_ok("deconvlist." + std::to_string(j) + ".residualnorm.", (double)Co * T * Fo)) return false;
        if (lvl > 0) {  // the skip output (decP[j]): the larger of its two branches (conv_weight_image.h: pair_skip_bound)
            auto rw = e->params.find("deconvlist." + std::to_string(j) + ".residual.weight"), rb = e->params.find("deconvlist." + std::to_string(j) + ".residual.bias");
            if (rw == e->params.end() || rb == e->params.end() || rw->second.size() != (size_t)Co * Co || rb->second.size() != (size_t)Co) return false;
            if (!(pair_skip_bound(rw->second.data(), rb->second.data(), Co, enc_bound[lvl - 1], dec_bound) <= kPairGuardLimit)) return false;
        }
    }
    if (!norm_ok("gru.norm.", (double)T * e->D)) return false;
    for (const auto &kv : e->params) {  // every weight operand: all *.weight / weight_* that are not a norm's gamma
        const std::string &k = kv.first;
        if (k.find("norm") != std::string::npos || k.find("weight") == std::string::npos) continue;
        float m = 0;
        if (!absmax(k, m) || m >= 16.0f) return false;
    }
    return true;
}

// whether this weight load runs the fp16 pair format: the knob, eligibility (precision 0, the CRN variant, the plane GEMM route's
// shapes) and the range guard
void f16_pair_decide(se_engine *e) {
    e->pair_on = e->f16_pair && e->precision == 0 && e->variant == 0 && gemm_p_capable(e) && f16_pair_guard(e);
}

int prepare_weights(se_engine *e) {
    if (e->weights_ready) return 0;
    std::string why;
    if (!crn_geometry_supported(e, &why)) return fail(e, SE_ERR_ARG, "%s", why.c_str());
    const int L = e->L, H = e->H, D = e->D;
    f16_pair_decide(e);
    // the norm affines of every level (the convolutions themselves are planned in prepare_weights_p)
    for (int i = 0; i < L; i++) {
        const int Co = e->Ch[i + 1];
        const std::string p = "convlist." + std::to_string(i) + ".";
        auto *nw = param(e, p + "norm.weight", Co);
        auto *nb = param(e, p + "norm.bias", Co);
        if (!nw || !nb) return SE_ERR_PARAM_MISSING;
        int rc;
        if ((rc = dev_upload(e, e->lv[i].enc_nw, *nw))) return rc;
        if ((rc = dev_upload(e, e->lv[i].enc_nb, *nb))) return rc;
    }
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j;
        const int Co = lvl == 0 ? 2 : e->Ch[lvl];
        const std::string p = "deconvlist." + std::to_string(j) + ".";
        auto *nw = param(e, p + "norm.weight", Co);
        auto *nb = param(e, p + "norm.bias", Co);
        if (!nw || !nb) return SE_ERR_PARAM_MISSING;
        int rc;
        if ((rc = dev_upload(e, e->lv[j].dec_nw, *nw))) return rc;
        if ((rc = dev_upload(e, e->lv[j].dec_nb, *nb))) return rc;
        if (lvl > 0) {  // skip path (CRN.py:485-487): the residualnorm affine of the gate (the 1x1 pair is planned in prepare_weights_p)
            auto *mnw = param(e, p + "residualnorm.weight", Co);
            auto *mnb = param(e, p + "residualnorm.bias", Co);
            if (!mnw || !mnb) return SE_ERR_PARAM_MISSING;
            if ((rc = dev_upload(e, e->lv[j].dec_mnw, *mnw))) return rc;
            if ((rc = dev_upload(e, e->lv[j].dec_mnb, *mnb))) return rc;
        }
    }
    for (int i = 0; i < e->npre; i++) {  // CRN_ELU.py:335-340: Conv2d(5x5, dilation (fd,1), padding (2fd,4)) + gated pair + gLN
        const int C0 = e->Ch[0], F0 = e->F[0], fd = 1 << i;
        const std::string p = "preconvlist." + std::to_string(i) + ".";
        auto *w = param(e, p + "conv.weight", (size_t)C0 * C0 * 25);
        auto *b = param(e, p + "conv.bias", C0);
        auto *tw = param(e, p + "conv_trans.weight", (size_t)C0 * C0);
        auto *tb = param(e, p + "conv_trans.bias", C0);
        auto *gw = param(e, p + "conv_gated.weight", (size_t)C0 * C0);
        auto *gb = param(e, p + "conv_gated.bias", C0);
        auto *nw = param(e, p + "norm.weight", C0);
        auto *nb = param(e, p + "norm.bias", C0);
        if (!w || !b || !tw || !tb || !gw || !gb || !nw || !nb) return SE_ERR_PARAM_MISSING;
        std::vector<std::array<int, 4>> taps;
        for (int kf = 0; kf < 5; kf++)
            for (int kt = 0; kt < 5; kt++) taps.push_back({kf, kt, kt, kf * fd});
        const float *wp = w->data(), *twp = tw->data(), *gwp = gw->data();
        int rc = plan_conv(e, e->lv[i].pre, C0, C0, F0, F0, F0, 1, 1, 0, 2 * fd, -4, 5, 1, F0 + 4 * fd, taps,
                           [=](int ci, int co, int kf, int kt) { return wp[(((size_t)co * C0 + ci) * 5 + kf) * 5 + kt]; }, *b, 0, C0, 2);
        if (rc) return rc;
        e->lv[i].pre.flops = 2.0 * C0 * C0 * 25 * F0 * e->T;
        {  // the gated 1x1 pair is fused into the conv's epilogue (all 5 channels of a position sit in one thread)
            std::vector<float> g;
            g.insert(g.end(), twp, twp + (size_t)C0 * C0);
            g.insert(g.end(), gwp, gwp + (size_t)C0 * C0);
            g.insert(g.end(), tb->begin(), tb->end());
            g.insert(g.end(), gb->begin(), gb->end());
            if ((rc = dev_upload(e, e->lv[i].pre.gatew, g))) return rc;
            e->lv[i].pre.lds += g.size() * sizeof(float);
            e->lv[i].pre.flops += 2.0 * 2 * C0 * C0 * F0 * e->T;
        }
        if ((rc = dev_upload(e, e->lv[i].pre_nw, *nw)) || (rc = dev_upload(e, e->lv[i].pre_nb, *nb))) return rc;
    }
    for (int l = 0; l < e->NL; l++) {
        const std::string s = std::to_string(l);
        const size_t in = l == 0 ? D : H;
        auto *a = param(e, "gru.sequence_model.weight_ih_l" + s, 3 * (size_t)H * in);
        auto *b = param(e, "gru.sequence_model.weight_hh_l" + s, 3 * (size_t)H * H);
        auto *c = param(e, "gru.sequence_model.bias_ih_l" + s, 3 * (size_t)H);
        auto *d = param(e, "gru.sequence_model.bias_hh_l" + s, 3 * (size_t)H);
        if (!a || !b || !c || !d) return SE_ERR_PARAM_MISSING;
        int rc;
        if ((rc = upload_planes(e, e->wih_x[l], *a, e->precision))) return rc;
        if ((rc = dev_upload(e, e->wih[l], *a)) || (rc = dev_upload(e, e->whh[l], *b)) ||
            (rc = dev_upload(e, e->bih[l], *c)) || (rc = dev_upload(e, e->bhh[l], *d)))
            return rc;
        if (e->pair_on && l > 0 && (rc = upload_planes_pair(e, e->wih_h[l], *a, pair_wplanes(e), kblock_on(e) ? (size_t)H : 0))) return rc;
        if (e->precision == 0 && H % 32 == 0) {
            std::vector<uint16_t> pk;
            if (e->pair_on && !e->pair_w3) gru_pack_whh_pair2(b->data(), H, pk);
            else if (e->pair_on) gru_pack_whh_pair(b->data(), H, pk);
            else gru_pack_whh(b->data(), H, pk);
            if ((rc = dev_alloc(e, e->whh_p[l], pk.size() / 2))) return rc;
            HIPCHECK(e, hipMemcpy(e->whh_p[l].p, pk.data(), pk.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        }
    }
    {
        auto *a = param(e, "gru.fc_output_layer.weight", (size_t)D * H);
        auto *b = param(e, "gru.fc_output_layer.bias", D);
        auto *c = param(e, "gru.norm.weight", D);
        auto *d = param(e, "gru.norm.bias", D);
        if (!a || !b || !c || !d) return SE_ERR_PARAM_MISSING;
        int rc;
        if ((rc = upload_planes(e, e->fcw_x, *a, e->precision))) return rc;
        if ((rc = dev_upload(e, e->fcw, *a)) || (rc = dev_upload(e, e->fcb, *b)) || (rc = dev_upload(e, e->gnw, *c)) ||
            (rc = dev_upload(e, e->gnb, *d)))
            return rc;
    }
    e->weights_ready = true;
    return 0;
}

int launch_conv(se_engine *e, const ConvPlan &pl, const float *x, const float *xprev, float *y, hipStream_t st, const char *label,
                float *stats = nullptr, int nslot = 0, int slot0 = 0, int stats_lo = 0, int stats_hi = 0) {
    if (!pl.active) return 0;
    // algorithmic MACs of this launch as SURVEY.md 8d counts them are attributed by the caller via pl.flops
    ProfScope ps(e, "k_conv_small", label, pl.flops * e->B, st);
    ConvArgs a = pl.a;
    a.x = x; a.xprev = xprev; a.y = y; a.w = pl.w.p; a.bias = pl.bias.p; a.gatew = pl.gatew.p;
    a.stats = stats; a.stats_nslot = nslot; a.stats_slot0 = slot0; a.stats_lo = stats_lo; a.stats_hi = stats_hi;
    dim3 grid(pl.grid_x, e->B);
    if (conv_igemm_launch(a.ntap, /*NT=*/0, a.CoPad, grid, pl.lds, st, a))  // NT 0: the vector-ALU instances
        return fail(e, SE_ERR_ARG, "no small conv kernel instance for %d taps", a.ntap);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

int launch_gemm(se_engine *e, const float *A, long lda, const float *W, long ldw, const float *bias, float *C, long ldc,
                int Mr, int Nc, int Kd, int relu, hipStream_t st, const char *label, const float *Wx = nullptr) {
    if (Mr <= e->skinny_rows && lda == Kd && ldw == Kd && Kd % 8 == 0) {  // few rows: 32 x 32 tiles, K split over the waves (fp32-exact MFMA)
        ProfScope ps(e, "k_gemm_skinny", label, 2.0 * Mr * Nc * Kd, st);
        if (se_train_gemm(A, W, bias, C, Mr, Nc, Kd, relu, st)) return fail(e, SE_ERR_HIP, "skinny GEMM launch failed: %s", se_train_last_error());
        return 0;
    }
    dim3 ggrid((Nc + kGemmBN - 1) / kGemmBN, (Mr + kGemmBM - 1) / kGemmBM);
    if (Wx && Kd % 8 == 0 && Kd >= 8 && lda % 4 == 0 && ldw == Kd) {
        ProfScope ps(e, e->precision == 1 ? "k_gemm_f16" : (e->precision == 2 ? "k_gemm_bf16x3" : "k_gemm_bf16x6"), label, 2.0 * Mr * Nc * Kd, st);
        GemmX6Args g{A, reinterpret_cast<const __bf16 *>(Wx), bias, C, Mr, Nc, Kd, lda, ldc, relu};
        if (e->precision == 1) hipLaunchKernelGGL(k_gemm_x<1>, ggrid, dim3(256), 0, st, g);
        else if (e->precision == 2) hipLaunchKernelGGL(k_gemm_x<2>, ggrid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL(k_gemm_x<3>, ggrid, dim3(256), 0, st, g);
        HIPCHECK(e, hipGetLastError());
        return 0;
    }
    ProfScope ps(e, "k_gemm_tn", label, 2.0 * Mr * Nc * Kd, st);
    if (Kd % 4 || Kd < 4 || lda % 4 || ldw % 4) return fail(e, SE_ERR_ARG, "GEMM inner dimension %d must be a multiple of 4", Kd);
    GemmArgs g{A, W, bias, C, Mr, Nc, Kd, lda, ldw, ldc, relu};
    dim3 grid((Nc + kGemmBN - 1) / kGemmBN, (Mr + kGemmBM - 1) / kGemmBM);
    hipLaunchKernelGGL(k_gemm_tn, grid, dim3(256), 0, st, g);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// C = act(A W^T + bias) with both operands as split-bf16 planes ([PL][rows][K] bf16, K % 32 == 0): k_gemm_p
int launch_gemm_p(se_engine *e, const float *Ap, const float *Wp, const float *bias, float *C, long ldc, int Mr, int Nc, int Kd, int relu,
                  hipStream_t st, const char *label, float *stats = nullptr) {
    // every plane GEMM is a bottleneck GEMM: A is gruinP or seqP (kGemmA), W the matching weight planes (the pair's stored planes: two, or three
    // under SE_PAIR_W3)
    const bool pair = buffer_format(e->precision, e->pair_on, PlaneBuf::kGemmA) == PlaneFmt::kF16Pair;
    const int PL = pair ? pair_wplanes(e) : operand_planes(e->precision), PA = buffer_planes(e->precision, e->pair_on, PlaneBuf::kGemmA);
    // (the profile record names the instance: "_w2" = the pair's two stored weight planes; tests tell the routes apart by it)
    ProfScope ps(e, pair && PL == kPairPlanesW2 ? "k_gemm_p_w2" : "k_gemm_p", label, 2.0 * Mr * Nc * Kd, st);
    const int nrt = (Mr + kGemmPBM - 1) / kGemmPBM, nct = (Nc + kGemmPBN - 1) / kGemmPBN;
    // XCD blocks: the split of the tile grid into 8 equal blocks (gx x gy) that fetches the fewest bytes into the 8 private
    // L2s - every row tile of A is fetched by the gy XCDs of its block row, every column tile of W by gx
    int gx = 0, gy = 0;
    double best = 0;
    for (int cx : {1, 2, 4, 8}) {
        if (nrt % cx || nct % (8 / cx)) continue;
        const double bytes = (double)Mr * (8 / cx) + (double)Nc * cx;  // x Kd x bytes per element, common to all candidates
        if (!gx || bytes < best) { gx = cx; gy = 8 / cx; best = bytes; }
    }
    int nblocks = nrt * nct;
    if (!gx && nrt * nct >= 16) {
        // no equal 8-block split divides the tile grid (B = 256: 21 x 12 tiles): block id -> XCD is id mod 8, so plain row-major order
        // hands every row tile of A to all eight L2s.  Banded: XCD x takes the `per` consecutive tiles [x per, (x + 1) per)
        const int per = (nrt * nct + 7) / 8;
        gx = -1; gy = per;
        nblocks = 8 * per;
    }
    // the A planes are laid out for the ALLOCATION batch ([PL][B * T][K]); a ragged call multiplies a prefix of the rows only (Mr = Bact * T)
    const long Ma = std::max<long>(Mr, (long)e->B * e->T);
    GemmPArgs g{reinterpret_cast<const uint4 *>(Ap), reinterpret_cast<const uint4 *>(Wp), Ma * Kd / 8, (long)Nc * Kd / 8, bias, C, Mr, Nc, Kd, ldc, relu,
                (unsigned)((size_t)PA * Ma * Kd * 2), (unsigned)((size_t)PL * Nc * Kd * 2), nrt, nct, gx, gy, stats};
    const dim3 grid(nblocks);
    const size_t lds = (size_t)2 * (1024 * PA + 512 * PL) * 16;
    // (K-blocked operands: the same buffers, ranges and stage size, whole rows of 2 K fp16 instead of planes)
    if (pair && PL == kPairPlanesW2 && kblock_on(e)) hipLaunchKernelGGL((k_gemm_p<kPairPlanesW2, PlaneFmt::kF16Pair, true>), grid, dim3(512), lds, st, g);
    else if (pair && PL == kPairPlanesW2) hipLaunchKernelGGL((k_gemm_p<kPairPlanesW2, PlaneFmt::kF16Pair>), grid, dim3(512), lds, st, g);
    else if (pair) hipLaunchKernelGGL((k_gemm_p<kPairPlanesW, PlaneFmt::kF16Pair>), grid, dim3(512), lds, st, g);
    else if (PL == 1) hipLaunchKernelGGL(k_gemm_p<1>, grid, dim3(512), lds, st, g);
    else if (PL == 2) hipLaunchKernelGGL(k_gemm_p<2>, grid, dim3(512), lds, st, g);
    else hipLaunchKernelGGL(k_gemm_p<3>, grid, dim3(512), lds, st, g);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

int launch_gln_ew(se_engine *e, const float *x, float *y, const float *w, const float *b, const float *slab, int nslot, long n,
                  int mode, int C, int T, int F, hipStream_t st, const float *res = nullptr) {
    ProfScope ps(e, "k_gln_ew", "gln", 0, st);
    GlnEwArgs g{x, y, w, b, SlabStats{slab, nslot, n, e->eps_mode}, mode, C, T, F, res};
    // grid-stride loop: about 8 workgroups per CU over the whole batch (every workgroup first reduces the producer's partial
    // statistics, so thousands of 4-element-per-thread workgroups per launch spent their time there)
    const int want = std::max(1, (8 * e->num_cu + e->B - 1) / e->B);
    if (n % 4 == 0) {
        const int gx = std::min((int)((n / 4 + 255) / 256), want);
        hipLaunchKernelGGL(k_gln_ew<4>, dim3(gx, e->B), dim3(256), 0, st, g);
    } else {
        const int gx = std::min((int)((n + 255) / 256), want);
        hipLaunchKernelGGL(k_gln_ew<1>, dim3(gx, e->B), dim3(256), 0, st, g);
    }
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// TemporalCRN.forward on device in three stages (stage_encoder_p, the bottleneck below, stage_decoder_p); each reads/writes the
// ring slot `cur` (history from slot `prev`).  spec: (b, m, t, f) strides; out: (b, t, f) strides (cf2 units).
// CRN_ELU / student with the pre-conv blocks on the vector-ALU kernel (convp_engine.inc.h: all but fp16 operands): features
// (CRN.py:463-467) and the three frequency-dilated pre-conv blocks -> pre_out (fp32)
int stage_features_pre(se_engine *e, int cur, const cf2 *spec, long sB, long sM, long sT, long sF, hipStream_t st) {
    const int T = e->T, B = e->B;
    int rc;
    e->parity ^= 1;
    const int pcur = e->parity, pprev = pcur ^ 1;
    {
        ProfScope ps(e, "k_featurize", "featurize", 0, st);
        FeatArgs f{spec, sB, sM, sT, sF, e->pin[0][pcur].p, e->M, T, e->F[0], e->atan2_phase};
        const int TF = T * e->F[0];
        hipLaunchKernelGGL(k_featurize, dim3((TF + 255) / 256, B), dim3(256), 0, st, f);
        HIPCHECK(e, hipGetLastError());
    }
    for (int i = 0; i < e->npre; i++) {  // x = m(x) + x, three frequency-dilated blocks (CRN_ELU.py:375-376)
        const int C0 = e->Ch[0], F0 = e->F[0];
        const long n = (long)C0 * T * F0;
        const int ns = e->lv[i].pre.grid_x;
        if ((rc = launch_conv(e, e->lv[i].pre, e->pin[i][pcur].p, e->pin[i][pprev].p, e->pre_g.p, st, ("pre" + std::to_string(i)).c_str(),
                              e->pre_stats[i].p, ns, 0, 0, C0))) return rc;
        float *dst = i + 1 < e->npre ? e->pin[i + 1][pcur].p : e->pre_out.p;
        if ((rc = launch_gln_ew(e, e->pre_g.p, dst, e->lv[i].pre_nw.p, e->lv[i].pre_nb.p, e->pre_stats[i].p, ns, n, 0, C0, T, F0, st,
                                e->pin[i][pcur].p))) return rc;
    }
    return 0;
}

uint4 *decin_p(se_engine *e, int slot);  // convp_engine.inc.h: decoder-input ring slot of the plane path

// Stage 2: the recurrent bottleneck (CRN.py:476-481, 256-282)  gruinP[cur] (or gru_in[cur]) -> decinP[cur]
// The bottleneck is cut where its data dependencies are (CRN.py:256-282):
//   stage_gru_proj0  x W_ih0^T for all T frames: depends only on the encoder output, so it runs on the ENCODER stream
//   stage_gru_layer  layer l: (l > 0: input projection of layer l-1's sequence) + T dependent step launches; each layer has
//                    its own stream in the pipelined path - layer 1 of segment n runs beside layer 0 of segment n+1
//   stage_gru_out    fc_output_layer + activation + gLN(last): depends only on the last layer's sequence: DECODER stream
// so the chain of dependent launches per segment is T steps (+ one GEMM) per stream instead of 2 T + 3 GEMMs on one stream.
// `overlapped`: the stage shares the chip with the other streams.  The GRU step then uses the small-footprint kernel
// (k_gru_step: 54 VGPRs, 6 KB LDS, W_hh straight from L2) whose waves fit next to resident convolution workgroups, instead
// of k_gru_step2 (188 VGPRs, 96 KB LDS slice of W_hh), which is 15 % faster alone but has to wait for a convolution
// workgroup to retire on every CU at every step.  On the plane GEMM route at precision 0 the overlapped stage runs the split-bf16
// step instead (k_gru_step_split: bf16 MFMAs on the planes of h_{t-1}, 200 registers, 12 KB LDS; SE_GRU_SPLIT, gru_split_on).
int stage_gru_proj0(se_engine *e, int cur, hipStream_t st) {
    const int T = e->T, B = e->B, H = e->H, D = e->D;
    if (e->dbg_skip & 2) return 0;
    const int Ba = e->Bact;
    (void)B;
    if (e->gemm_p) return launch_gemm_p(e, e->gruinP[cur].p, e->wih_xp.p, e->bih[0].p, e->gi0[cur].p, 3L * H, Ba * T, 3 * H, D, 0, st, "gru_ih0");
    return launch_gemm(e, e->gru_in[cur].p, D, e->wih[0].p, D, e->bih[0].p, e->gi0[cur].p, 3L * H, Ba * T, 3 * H, D, 0, st, "gru_ih0", e->wih_x[0].p);
}

// W_ih of layer l >= 1 as the plane GEMM reads it
const float *wih_planes(const se_engine *e, int l) { return e->pair_on ? e->wih_h[l].p : e->wih_x[l].p; }
// the sequence planes of a step's arguments at time step t: seqP slot `base` ([PL][B * T][H] for the allocation batch B, or K-blocked
// rows of 2 H), plane count and format
void set_seqp(const se_engine *e, GruStepArgs &g, float *base, int t) {
    const long T = e->T, H = e->H, B = e->B;
    g.seqp_pl = buffer_planes(e->precision, e->pair_on, PlaneBuf::kGemmA);
    g.seqp_pair = buffer_format(e->precision, e->pair_on, PlaneBuf::kGemmA) == PlaneFmt::kF16Pair;
    g.seqp_kb = kblock_on(e);
    const long row = g.seqp_kb ? 2 * H : H;  // elements per (stream, time step)
    g.seqp = reinterpret_cast<__bf16 *>(base) + t * row;
    g.seqp_ld = T * row;
    g.seqp_plane = g.seqp_kb ? kKbBlock : B * T * H;
}
// row t - 1 of the same planes: h_{t-1} as the split step reads it (t >= 1)
const __bf16 *seqp_prev(const GruStepArgs &g, int H) { return g.seqp - (g.seqp_kb ? 2 * H : H); }

// The split-bf16 step (k_gru_step_split) reads h_{t-1} as the planes the plane GEMM route writes and W_hh as packed PL = 3 fragments
bool gru_split_eligible(const se_engine *e) { return e->gemm_p && e->precision == 0 && e->H % 32 == 0 && e->B > 16; }
bool gru_split_on(const se_engine *e, bool overlapped) {
    if (!gru_split_eligible(e) || e->gru_split == 0) return false;
    return e->gru_split == 1 || (overlapped && e->gru_direct < 0);
}
// (32 streams per workgroup, two k steps in flight per wave: the variant that won in the pipelined step, gemm.hip.h)
void launch_gru_split(se_engine *e, const GruSplitArgs &g, int rows, hipStream_t st) {
    if (e->pair_on && !e->pair_w3) hipLaunchKernelGGL((k_gru_step_split<1, 2, true, kPairPlanesW2>), dim3(e->H / 32, (rows + 31) / 32), dim3(256), 0, st, g);
    else if (e->pair_on) hipLaunchKernelGGL((k_gru_step_split<1, 2, true>), dim3(e->H / 32, (rows + 31) / 32), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((k_gru_step_split<1, 2>), dim3(e->H / 32, (rows + 31) / 32), dim3(256), 0, st, g);
}
void launch_gru_split_multi(se_engine *e, const GruSplitMulti &m, int rows, int z, hipStream_t st) {
    if (e->pair_on && !e->pair_w3) hipLaunchKernelGGL((k_gru_step_split_multi<1, 2, true, kPairPlanesW2>), dim3(e->H / 32, (rows + 31) / 32, z), dim3(256), 0, st, m);
    else if (e->pair_on) hipLaunchKernelGGL((k_gru_step_split_multi<1, 2, true>), dim3(e->H / 32, (rows + 31) / 32, z), dim3(256), 0, st, m);
    else hipLaunchKernelGGL((k_gru_step_split_multi<1, 2>), dim3(e->H / 32, (rows + 31) / 32, z), dim3(256), 0, st, m);
}

int stage_gru_layer(se_engine *e, int l, int cur, hipStream_t st, bool overlapped) {
    const int T = e->T, B = e->B, H = e->H;
    const int Ba = e->Bact;  // rows that take part (prefix of the batch)
    int rc;
    const float *gi = e->gi0[cur].p;
    if (l > 0) {
        gi = e->gil[l].p;
        if (e->dbg_skip & 2) {}
        else if (e->gemm_p) { if ((rc = launch_gemm_p(e, e->seqP[l - 1][cur].p, wih_planes(e, l), e->bih[l].p, e->gil[l].p, 3L * H, Ba * T, 3 * H, H, 0, st, ("gru_ih" + std::to_string(l)).c_str()))) return rc; }
        else if ((rc = launch_gemm(e, e->seqr[l - 1][cur].p, H, e->wih[l].p, H, e->bih[l].p, e->gil[l].p, 3L * H, B * T, 3 * H, H, 0, st,
                                   ("gru_ih" + std::to_string(l)).c_str(), e->wih_x[l].p))) return rc;
    }
    float *seq = e->seqr[l][cur].p;
    const bool split = gru_split_on(e, overlapped);
    for (int t = 0; t < T && !(e->dbg_skip & 1); t++) {
        const int hc = e->hcur[l];
        GruStepArgs g{gi + (long)t * 3 * H, (long)T * 3 * H, e->hbuf[l][hc].p, e->whh[l].p, e->bhh[l].p,
                      e->hbuf[l][hc ^ 1].p, seq + (long)t * H, (long)T * H, Ba, H};
        if (e->gemm_p) set_seqp(e, g, e->seqP[l][cur].p, t);
        if (split) {
            ProfScope ps(e, e->pair_on && !e->pair_w3 ? "k_gru_step_split_w2" : "k_gru_step_split", "gru_step", 2.0 * B * 3 * H * H, st);
            launch_gru_split(e, GruSplitArgs{g, reinterpret_cast<const uint4 *>(e->whh_p[l].p), t ? seqp_prev(g, H) : nullptr}, Ba, st);
            e->hcur[l] = hc ^ 1;
            continue;
        }
        ProfScope ps(e, "k_gru_step", "gru_step", 2.0 * B * 3 * H * H, st);
        const dim3 grid((H + 15) / 16, (Ba + 31) / 32);
        // (<= 16 streams: the register-streaming kernel splits K over all four waves and beats the LDS-slice kernel: 9.3 vs 10.4 us)
        const bool direct = e->gru_direct >= 0 ? e->gru_direct != 0 : (overlapped || B <= 16);
        if (H == 512 && !direct) hipLaunchKernelGGL(k_gru_step2<16>, grid, dim3(256), (size_t)192 * H, st, g);
        else if (H == 128 && !direct) hipLaunchKernelGGL(k_gru_step2<4>, grid, dim3(256), (size_t)192 * H, st, g);
        else if (B <= 16) hipLaunchKernelGGL(k_gru_step8, grid, dim3(512), 0, st, g);
        else hipLaunchKernelGGL(k_gru_step, grid, dim3(256), 0, st, g);
        e->hcur[l] = hc ^ 1;
    }
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// Pipelined form of the recurrence: ONE stream, layer l works on the segment in ring slot slots[l] (-1: none).  Layer l lags
// l segments behind layer 0, so the steps of all layers of a round are independent of each other and every time step is ONE
// launch (k_gru_step_multi, blockIdx.z = layer) instead of one per layer: T dependent launches per segment instead of NL * T.
int stage_gru_round(se_engine *e, const int *slots, hipStream_t st) {
    const int T = e->T, B = e->B, H = e->H;
    int rc;
    const float *gi[4] = {nullptr, nullptr, nullptr, nullptr};
    int nact = 0;
    for (int l = 0; l < e->NL; l++) {
        if (slots[l] < 0) continue;
        nact++;
        gi[l] = e->gi0[slots[l]].p;
        if (l > 0) {
            gi[l] = e->gil[l].p;
            if (e->dbg_skip & 2) {}
            else if (e->gemm_p) { if ((rc = launch_gemm_p(e, e->seqP[l - 1][slots[l]].p, wih_planes(e, l), e->bih[l].p, e->gil[l].p, 3L * H, e->bact_slot[slots[l]] * T, 3 * H, H, 0, st, ("gru_ih" + std::to_string(l)).c_str()))) return rc; }
            else if ((rc = launch_gemm(e, e->seqr[l - 1][slots[l]].p, H, e->wih[l].p, H, e->bih[l].p, e->gil[l].p, 3L * H, B * T, 3 * H, H, 0, st,
                                       ("gru_ih" + std::to_string(l)).c_str(), e->wih_x[l].p))) return rc;
        }
    }
    if (!nact) return 0;
    int bmax = 0;  // every layer's own row count is in its arguments; the grid covers the largest
    for (int l = 0; l < e->NL; l++)
        if (slots[l] >= 0) bmax = std::max(bmax, e->bact_slot[slots[l]]);
    const bool split = gru_split_on(e, /*overlapped=*/true);
    for (int t = 0; t < T && !(e->dbg_skip & 1); t++) {
        GruStepMulti m{};
        GruSplitMulti ms{};
        int z = 0;
        for (int l = 0; l < e->NL; l++) {
            if (slots[l] < 0) continue;
            const int hc = e->hcur[l];
            GruStepArgs &ga = m.a[z++];
            ga = GruStepArgs{gi[l] + (long)t * 3 * H, (long)T * 3 * H, e->hbuf[l][hc].p, e->whh[l].p, e->bhh[l].p,
                             e->hbuf[l][hc ^ 1].p, e->seqr[l][slots[l]].p + (long)t * H, (long)T * H, e->bact_slot[slots[l]], H};
            if (e->gemm_p) set_seqp(e, ga, e->seqP[l][slots[l]].p, t);
            e->hcur[l] = hc ^ 1;
            if (split) ms.a[z - 1] = GruSplitArgs{ga, reinterpret_cast<const uint4 *>(e->whh_p[l].p), t ? seqp_prev(ga, H) : nullptr};
        }
        if (split) {
            ProfScope ps(e, e->pair_on && !e->pair_w3 ? "k_gru_step_split_multi_w2" : "k_gru_step_split_multi", "gru_step", 2.0 * B * 3 * H * H * z, st);
            launch_gru_split_multi(e, ms, bmax, z, st);
            continue;
        }
        ProfScope ps(e, "k_gru_step", "gru_step", 2.0 * B * 3 * H * H * z, st);
        // (the same arithmetic as the single-stream path: batches of <= 16 streams split K over eight waves)
        if (B <= 16) hipLaunchKernelGGL(k_gru_step_multi8, dim3((H + 15) / 16, 1, z), dim3(512), 0, st, m);
        else hipLaunchKernelGGL(k_gru_step_multi, dim3((H + 15) / 16, (bmax + 31) / 32, z), dim3(256), 0, st, m);
    }
    HIPCHECK(e, hipGetLastError());
    return 0;
}

int stage_gru_out(se_engine *e, int cur, hipStream_t st) {
    const int L = e->L, T = e->T, B = e->B, H = e->H, D = e->D;
    const int Ba = e->Bact;
    (void)B;
    int rc;
    // decoder input in the plane layout
    const int PL = operand_planes(e->precision), C = e->Ch[L], C8 = (C + 7) / 8, Fl = e->F[L];
    const PlaneFmt dfmt = act_format(e, PlaneBuf::kConvAct);  // decinP
    Gln2PArgs g{e->fc_out.p, e->gnw.p, e->gnb.p, decin_p(e, cur), (long)C8 * act_planes(e, PlaneBuf::kConvAct) * T * Fl, T, Fl, C, C8, e->eps_mode, SlabStats{}};
    if (e->gemm_p) {  // octet-interleaved columns, statistics from the GEMM's epilogue, full-chip one-pass norm
        const int ND = C8 * Fl * 8, nct = (ND + kGemmPBN - 1) / kGemmPBN;
        if (!(e->dbg_skip & 2) && (rc = launch_gemm_p(e, e->seqP[e->NL - 1][cur].p, e->fcw_xp.p, e->fcb_p.p, e->fc_out.p, ND, Ba * T, ND, H, e->act, st, "gru_fc", e->fc_stats.p))) return rc;
        ProfScope ps(e, "k_gln2_p", "gln_fc", 0, st);  // (records are keyed by label: its own, not the conv norms' "gln")
        g.w = e->gnw_p.p; g.b = e->gnb_p.p;
        g.st = SlabStats{e->fc_stats.p, T * nct, (long)T * C * Fl, e->eps_mode};
        launch_k_gln2_p(PL, dim3((T * Fl + 1023) / 1024, C8, Ba), st, g, dfmt);
        HIPCHECK(e, hipGetLastError());
        return 0;
    }
    // fp32 GEMM route (few rows): the reference's column order, two-pass statistics in the norm kernel
    if (!(e->dbg_skip & 2) && (rc = launch_gemm(e, e->seqr[e->NL - 1][cur].p, H, e->fcw.p, H, e->fcb.p, e->fc_out.p, D, Ba * T, D, H, e->act, st, "gru_fc", e->fcw_x.p))) return rc;
    ProfScope ps(e, "k_gln2_stream_p", "gln_fc_stream", 0, st);
    launch_k_gln2_stream_p(PL, dim3(Ba), st, g, dfmt);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// single-stream form: all bottleneck stages back to back
int stage_bottleneck(se_engine *e, int cur, hipStream_t st, bool overlapped = false) {
    int rc;
    if ((rc = stage_gru_proj0(e, cur, st))) return rc;
    for (int l = 0; l < e->NL; l++)
        if ((rc = stage_gru_layer(e, l, cur, st, overlapped))) return rc;
    return stage_gru_out(e, cur, st);
}

}  // namespace

#include "convp_engine.inc.h"

namespace {

int run_encoder(se_engine *e, int cur, int prev, const cf2 *spec, long sB, long sM, long sT, long sF, hipStream_t st, bool feat_done = false) {
    if (e->dbg_skip & 4) return 0;
    return stage_encoder_p(e, cur, prev, spec, sB, sM, sT, sF, st, feat_done);
}
int run_decoder(se_engine *e, int cur, const cf2 *spec, long sB, long sT, long sF, cf2 *out, long oB, long oT, long oF, hipStream_t st,
                float *wav = nullptr, long wav_ld = 0) {
    if (e->dbg_skip & 8) return 0;
    return stage_decoder_p(e, cur, spec, sB, sT, sF, out, oB, oT, oF, st, wav, wav_ld);
}

int forward_dev(se_engine *e, const cf2 *spec, long sB, long sM, long sT, long sF, cf2 *out, long oB, long oT, long oF,
                hipStream_t st) {
    const int prev = e->slot, cur = (e->slot + 1) % kRing;
    e->slot = cur;
    int rc;
    if ((rc = run_encoder(e, cur, prev, spec, sB, sM, sT, sF, st))) return rc;
    if ((rc = stage_bottleneck(e, cur, st))) return rc;
    return run_decoder(e, cur, spec, sB, sT, sF, out, oB, oT, oF, st);
}

// k_stft / k_istft on the engine's signal chain (sig_chain.h), timed and with the engine's error text.  rows: the per-stream lengths and
// offsets of a chains call.  nseg > 1: one launch for nseg consecutive segments (segment y reads off + y*seg_off, writes spec + y*seg_spec)
int launch_stft(se_engine *e, const float *src, long strideB, long strideM, int M, long off, long Lsrc, SigRows rows, int nrows,
                cf2 *spec, long sR, long sT, long sF, hipStream_t st, int nseg = 1, long seg_off = 0, long seg_spec = 0) {
    ProfScope ps(e, "k_stft", "stft", 0, st);
    HIPCHECK(e, sig_stft(e->sig, src, strideB, strideM, M, off, Lsrc, rows, nrows, spec, sR, sT, sF, st, nseg, seg_off, seg_spec));
    return 0;
}

int launch_istft(se_engine *e, const cf2 *spec, long sR, long sT, long sF, int nrows, float *wav, long wav_ld, hipStream_t st,
                 int nseg = 1, long seg_spec = 0, long seg_wav = 0) {
    ProfScope ps(e, "k_istft", "istft", 0, st);
    HIPCHECK(e, sig_istft(e->sig, spec, sR, sT, sF, nrows, wav, wav_ld, st, nseg, seg_spec, seg_wav));
    return 0;
}

// The one place that decides the bottleneck GEMM route of the current batch: plane GEMMs (k_gemm_p) when the engine can run
// them AND the batch has more rows than the skinny fp32 kernel wins at.  Called after every re-plan and from se_reset.
void select_gemm_route(se_engine *e) { e->gemm_p = e->gemm_p_cap && e->B > 0 && (long)e->B * e->T > e->skinny_rows; }

int ensure_ready(se_engine *e) {
    if (!e) return SE_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    const bool replanned = !e->weights_ready;
    int rc = prepare_weights(e);
    if (rc) return rc;
    if (replanned) {
        // (convert_history_p: the conv history rings only.  gruinP and seqP carry nothing from call to call - the recurrent state is fp32
        // and is split at t = 0 - so a load that flips their format or their K-blocking needs no conversion: every launch derives
        // strides and layout from the engine's current flags)
        if ((rc = prepare_weights_p(e)) || (rc = convert_history_p(e))) return rc;
        // capability only: whether THIS batch takes the plane GEMMs is select_gemm_route()'s decision (a batch on the skinny route
        // never allocated gruinP / seqP, so a weight reload must not switch the plane route back on behind its back)
        e->gemm_p_cap = gemm_p_capable(e);
        select_gemm_route(e);
        if (e->gemm_p_cap) {  // W_ih0 with its K axis in the engine's feature order k' = (o * F + f) * 8 + c  (reference d = (8 o + c) * F + f)
            const int Fl = e->F[e->L], D = e->D, H = e->H;
            const std::vector<float> &w = e->params["gru.sequence_model.weight_ih_l0"];
            std::vector<float> wp((size_t)3 * H * D);
            for (int r = 0; r < 3 * H; r++)
                for (int d = 0; d < D; d++) {
                    const int cabs = d / Fl, f = d - cabs * Fl;
                    wp[(size_t)r * D + ((size_t)(cabs >> 3) * Fl + f) * 8 + (cabs & 7)] = w[(size_t)r * D + d];
                }
            if ((rc = e->pair_on ? upload_planes_pair(e, e->wih_xp, wp, pair_wplanes(e), kblock_on(e) ? (size_t)D : 0) : upload_planes(e, e->wih_xp, wp, e->precision))) return rc;
            // fc_output_layer rows, its bias and the affine of the norm behind it in the same order (each dot product is unchanged;
            // only where it lands changes), channels padded to whole octets with zero rows.  (gemm_p_cap above asks for whole
            // octets, so today ND == D and no padding row exists; the padding is what a relaxed cap would need, and is untested)
            const int Cl = e->Ch[e->L], ND = (Cl + 7) / 8 * Fl * 8;
            const std::vector<float> &fw = e->params["gru.fc_output_layer.weight"], &fb = e->params["gru.fc_output_layer.bias"];
            const std::vector<float> &nw = e->params["gru.norm.weight"], &nb = e->params["gru.norm.bias"];
            std::vector<float> fwp((size_t)ND * H, 0.0f), fbp(ND, 0.0f), nwp(ND, 0.0f), nbp(ND, 0.0f);
            for (int d = 0; d < D; d++) {
                const int cabs = d / Fl, f = d - cabs * Fl;
                const size_t dp = ((size_t)(cabs >> 3) * Fl + f) * 8 + (cabs & 7);
                std::copy(fw.begin() + (size_t)d * H, fw.begin() + (size_t)(d + 1) * H, fwp.begin() + dp * H);
                fbp[dp] = fb[d]; nwp[dp] = nw[d]; nbp[dp] = nb[d];
            }
            if ((rc = e->pair_on ? upload_planes_pair(e, e->fcw_xp, fwp, pair_wplanes(e), kblock_on(e) ? (size_t)H : 0) : upload_planes(e, e->fcw_xp, fwp, e->precision)) || (rc = dev_upload(e, e->fcb_p, fbp)) || (rc = dev_upload(e, e->gnw_p, nwp)) ||
                (rc = dev_upload(e, e->gnb_p, nbp)))
                return rc;
        }
        if (e->B > 0) {  // the tilings follow the buffer format, which this load may have flipped: slabs for the new grids
            select_all_p(e);
            if ((rc = alloc_stats_p(e))) return rc;
        }
    }
    return 0;
}

}  // namespace

namespace {
// R layout [b][C8][npos][8] fp32 (the pre-norm output of k_conv_p: a feature-tap re-run) -> [b][c][f][t], the reference's feature-map
// layout (distillation_crn.py:467-477).  (t, f) sits at position t * oT + f, or, parity-planar (Fh > 0: the two output-frequency
// parities of a transposed convolution side by side), at t * oT + (f & 1) * Fh + (f >> 1).  One thread per (b, octet, f, t): 32 bytes in,
// eight columns out, coalesced over t.
__global__ void k_tap_r_to_bcft(const float *R, float *dst, int B, int C, int T, int F, int oT, int Fh) {
    const int C8 = (C + 7) >> 3;
    const long n = (long)B * C8 * F * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i % T);
        long r = i / T;
        const int f = (int)(r % F);
        r /= F;
        const int o = (int)(r % C8);
        const long b = r / C8;
        const long pos = (long)t * oT + (Fh ? (f & 1) * Fh + (f >> 1) : f);
        const float4 *src = reinterpret_cast<const float4 *>(R + ((b * C8 + o) * (long)T * oT + pos) * 8);
        const float4 lo = src[0], hi = src[1];
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (o * 8 + c < C) dst[((b * C + o * 8 + c) * F + f) * T + t] = v[c];
    }
}
}  // namespace

// ---- WHERE a stream's carried state lives: f(live tensor, carry buffer, words per stream row) for every state tensor in `which` ----
// which: bit 0 = encoder rows (conv history of every level + preconv history) in ring slot e->slot / parity e->parity, bit (1 + l) = h of
// GRU layer l in its current half.  Stream b's row starts at live + b * words.  Stops at the first f that returns non-zero.
template <class F>
static int state_rows_of(se_engine *e, unsigned which, F &&f) {
    static_assert(SE_MAX_LEVELS + 3 + 4 <= kStateRowsMax, "state row table too small");
    int rc;
    if (which & 1u) {
        for (int i = 0; i < e->L; i++)  // [slot][b][C8][planes][T][F] pieces of 16 bytes; the stream stride follows the buffer's format
            if ((rc = f(e->cp->xinP[i].p + (size_t)e->slot * e->cp->slot_elems[i] * 4, e->carry_x[i], xin_stream_elems(e, i) * 4))) return rc;
        for (int i = 0; i < e->npre; i++) {
            if (e->cp->pre_p) rc = f(e->cp->pinP[i].p + (size_t)e->slot * e->cp->pslot_elems * 4, e->carry_p[i], (long)(e->cp->pslot_elems / e->B) * 4);
            else rc = f(e->pin[i][e->parity].p, e->carry_p[i], (long)e->Ch[0] * e->T * e->F[0]);
            if (rc) return rc;
        }
    }
    for (int l = 0; l < e->NL; l++)
        if ((which & (2u << l)) && (rc = f(e->hbuf[l][e->hcur[l]].p, e->carry_h[l], (long)e->H))) return rc;
    return 0;
}

extern "C" {

int se_abi_version(void) { return 5; }

int se_config_size(void) { return (int)sizeof(se_config); }
int fsn_config_size(void) { return (int)sizeof(fsn_config); }

const char *se_last_error(const se_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int se_create(const se_config *cfg, int device, se_engine **out) {
    if (!cfg || !out) return fail(nullptr, SE_ERR_ARG, "null argument");
    *out = nullptr;
    const int L = cfg->num_levels;
    if (L < 1 || L > SE_MAX_LEVELS) return fail(nullptr, SE_ERR_ARG, "num_levels %d out of range", L);
    if (cfg->kernel_size != 3) return fail(nullptr, SE_ERR_ARG, "kernel_size %d unsupported (reference config uses 3)", cfg->kernel_size);
    if (cfg->num_layers < 1 || cfg->num_layers > 4) return fail(nullptr, SE_ERR_ARG, "num_layers %d out of range", cfg->num_layers);
    if (cfg->hidden <= 0 || cfg->hidden % 16) return fail(nullptr, SE_ERR_ARG, "hidden must be a positive multiple of 16 (k_gru_step walks 16-deep k blocks)");
    if (cfg->n_fft % 2 || cfg->num_freqs != cfg->n_fft / 2 + 1) return fail(nullptr, SE_ERR_ARG, "num_freqs must be n_fft/2+1 (CRN.py:511)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SE_ERR_HIP, "no HIP device available: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, SE_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
    se_engine *e = new se_engine();
    e->c = *cfg;
    e->device = device;
    e->L = L; e->M = cfg->num_inputs; e->K = cfg->segment_length; e->N = cfg->n_fft; e->H = cfg->hidden; e->NL = cfg->num_layers;
    if (cfg->variant < 0 || cfg->variant > 2) { delete e; return fail(nullptr, SE_ERR_ARG, "variant %d unknown (0 CRN, 1 CRN_ELU, 2 student)", cfg->variant); }
    if (cfg->precision < 0 || cfg->precision > 2) { delete e; return fail(nullptr, SE_ERR_ARG, "precision %d unknown (0 fp32-accurate, 1 fp16 operands, 2 bf16x3)", cfg->precision); }
    e->precision = cfg->precision;
    e->variant = cfg->variant;
    e->act = cfg->variant ? 2 : 1;
    e->npre = cfg->variant ? 3 : 0;
    e->atan2_phase = cfg->variant == 1;
    e->eps_mode = cfg->variant == 2;
    auto bail = [&](int code, const char *msg) { g_create_error = msg; sig_chain_destroy(e->sig); delete e; return code; };
    {  // STFT geometry, tables and the FFT kernels' LDS opt-in
        std::string why;
        if (int rc = sig_chain_create(e->sig, cfg->n_fft, cfg->win, cfg->hop, cfg->segment_length, device, why)) return bail(rc, why.c_str());
    }
    e->T = e->sig.T;
    e->F[0] = cfg->num_freqs;
    e->Ch[0] = 2 * cfg->num_inputs - 1;
    for (int i = 0; i < L; i++) { e->F[i + 1] = (e->F[i] - 1) / 2 + 1; e->Ch[i + 1] = cfg->channels[i]; }
    e->D = (cfg->num_freqs / 16 + 1) * cfg->channels[L - 1];
    if (e->D != e->F[L] * cfg->channels[L - 1]) return bail(SE_ERR_ARG, "num_freqs/num_levels combination breaks the reference reshape (CRN.py:450,478)");
    if (e->T <= 2 * (1 << (L - 1))) return bail(SE_ERR_ARG, "segment shorter than the largest dilation history (CRN.py:333)");
    if (const char *s = getenv("SE_GRU_DIRECT")) e->gru_direct = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_GRU_SPLIT")) e->gru_split = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_F16_PAIR")) e->f16_pair = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_F16_PAIR_CONV")) e->f16_pair_conv = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_PAIR_W3")) e->pair_w3 = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_GEMM_KBLOCK")) e->gemm_kblock = atoi(s) != 0 ? 1 : 0;
    if (const char *s = getenv("SE_PIPELINE")) e->pipeline = atoi(s);
#ifdef SE_DEBUG_KNOBS  // timing-experiment build only (profiles/pipe_split.sh): drops whole stages, the audio is WRONG
    if (const char *s = getenv("SE_DBG_SKIP")) { e->dbg_skip = atoi(s); fprintf(stderr, "se_engine: SE_DBG_SKIP=%d - stages are skipped, results are WRONG (timing experiment)\n", e->dbg_skip); }
#else
    if (getenv("SE_DBG_SKIP")) return bail(SE_ERR_ARG, "SE_DBG_SKIP is set but this library was built without -DSE_DEBUG_KNOBS: refusing to run (the knob drops whole stages and produces wrong audio)");
#endif
    if (const char *s = getenv("SE_GEMM_P")) e->gemm_p_env = atoi(s);
    if (const char *s = getenv("SE_GEMM_SKINNY_ROWS")) e->skinny_rows = atoi(s);
    if (const char *s = getenv("SE_SKIP_MIN_BATCH")) e->skip_min_batch = atoi(s);
    if (const char *s = getenv("SE_SKIP_DEPTH")) e->skip_depth = atoi(s) > 0 ? atoi(s) : 0;
    if (const char *s = getenv("SE_DEC_PAIR")) e->dec_pair = atoi(s) != 0 ? 1 : 0;
    for (int j = 0; j < SE_MAX_LEVELS; j++) {
        const char *s = getenv(("SE_DEC_PAIR_dec" + std::to_string(j)).c_str());
        e->dec_pair_site[j] = s ? (atoi(s) != 0 ? 1 : 0) : -1;
    }
    if (const char *s = getenv("SE_IO_FUSE")) e->io_fuse = atoi(s) != 0 ? 1 : 0;
    e->io_fuse_on = e->io_fuse && sig_io_fused_fits(e->sig, e->M);
    e->cp = new se_convp_state();
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) e->num_cu = ncu;
    }
    conv_set_attributes();
    conv_p_set_attributes();
    skip_p_set_attributes();
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 1536 * 1 * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 1536 * 2 * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 1536 * 3 * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<kPairPlanesW, PlaneFmt::kF16Pair>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * (1024 * kPairPlanesA + 512 * kPairPlanesW) * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<kPairPlanesW2, PlaneFmt::kF16Pair>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * (1024 * kPairPlanesA + 512 * kPairPlanesW2) * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gemm_p<kPairPlanesW2, PlaneFmt::kF16Pair, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              2 * (1024 * kPairPlanesA + 512 * kPairPlanesW2) * 16);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gru_step2<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 192 * 512);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_gru_step2<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 192 * 128);
    *out = e;
    return SE_OK;
}

void se_destroy(se_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
#ifdef SE_CP_TRACE
    g_cp_trace_sites.dump();
#endif
    DevBuf *singles[] = {&e->fcw, &e->fcb, &e->gnw, &e->gnb, &e->maskspec,
                         &e->fcw_x, &e->wih_xp, &e->fcw_xp, &e->fcb_p, &e->gnw_p, &e->gnb_p, &e->fc_stats, &e->pre_g, &e->pre_out, &e->spec_all, &e->mask_all, &e->fc_out, &e->yseg};
    for (DevBuf *b : singles) dev_free(*b);
    dev_free(e->plan_dev);
    for (DevBuf &b : e->carry_x) dev_free(b);
    for (DevBuf &b : e->carry_p) dev_free(b);
    for (DevBuf &b : e->carry_h) dev_free(b);
    for (int r = 0; r < kRing; r++) {
        dev_free(e->spec[r]); dev_free(e->gru_in[r]); dev_free(e->gi0[r]); dev_free(e->gruinP[r]);
        for (int l = 0; l < 4; l++) dev_free(e->seqP[l][r]);
        for (int l = 0; l < 4; l++) dev_free(e->seqr[l][r]);
        if (e->stage_ready) { (void)hipEventDestroy(e->ev_enc[r]); (void)hipEventDestroy(e->ev_dec[r]); (void)hipEventDestroy(e->ev_gru[r]); }
    }
    if (e->stage_ready) {
        (void)hipEventDestroy(e->ev_fork); (void)hipEventDestroy(e->ev_join);
        for (hipStream_t q : e->stage_stream) (void)hipStreamDestroy(q);
    }
    for (int i = 0; i < 4; i++) {
        dev_free(e->wih[i]); dev_free(e->whh[i]); dev_free(e->whh_p[i]); dev_free(e->bih[i]); dev_free(e->bhh[i]); dev_free(e->wih_x[i]); dev_free(e->wih_h[i]);
        dev_free(e->hbuf[i][0]); dev_free(e->hbuf[i][1]); dev_free(e->gil[i]);
    }
    for (int i = 0; i < SE_MAX_LEVELS; i++) {
        Level &l = e->lv[i];
        dev_free(l.pre.w); dev_free(l.pre.bias); dev_free(l.pre.gatew);
        for (DevBuf *b : {&l.enc_nw, &l.enc_nb, &l.dec_nw, &l.dec_nb, &l.dec_mnw, &l.dec_mnb}) dev_free(*b);
        dev_free(e->enc_stats[i]); dev_free(e->dec_stats[i]); dev_free(e->skip_stats[i]);
        dev_free(l.pre_nw); dev_free(l.pre_nb);
        if (i < 3) { dev_free(e->pin[i][0]); dev_free(e->pin[i][1]); dev_free(e->pre_stats[i]); }
    }
    free_state_p(e);
    sig_chain_destroy(e->sig);
    delete e;
}

int se_load_param(se_engine *e, const char *key, const float *host_data, const int64_t *shape, int ndim) {
    if (!e || !key || !host_data) return fail(e, SE_ERR_ARG, "null argument");
    const std::string k = canon(key);
    // accept exactly the reference's key set
    int idx = -1, n = 0;
    char rest[64];
    bool ok = false;
    auto gated_key = [&](const char *r) {
        return e->variant && (!strcmp(r, "conv_trans.weight") || !strcmp(r, "conv_trans.bias") || !strcmp(r, "conv_gated.weight") || !strcmp(r, "conv_gated.bias"));
    };
    if (sscanf(k.c_str(), "preconvlist.%d.%63s", &idx, rest) == 2)
        ok = e->variant && idx >= 0 && idx < 3 && (!strcmp(rest, "conv.weight") || !strcmp(rest, "conv.bias") || !strcmp(rest, "norm.weight") || !strcmp(rest, "norm.bias") || gated_key(rest));
    else if (sscanf(k.c_str(), "convlist.%d.%63s", &idx, rest) == 2)
        ok = idx >= 0 && idx < e->L && (!strcmp(rest, "conv.weight") || !strcmp(rest, "conv.bias") || !strcmp(rest, "norm.weight") || !strcmp(rest, "norm.bias") || gated_key(rest));
    else if (sscanf(k.c_str(), "deconvlist.%d.%63s", &idx, rest) == 2) {
        static const char *names[] = {"conv.weight", "conv.bias", "norm.weight", "norm.bias", "residualmask.weight", "residualmask.bias",
                                      "residualnorm.weight", "residualnorm.bias", "residual.weight", "residual.bias"};
        for (const char *nm : names) ok = ok || !strcmp(rest, nm);
        ok = ok && idx >= 0 && idx < e->L;
    } else if (sscanf(k.c_str(), "gru.sequence_model.%63[a-z_]%d%n", rest, &idx, &n) == 2)
        ok = idx >= 0 && idx < e->NL && (size_t)n == k.size() &&
             (!strcmp(rest, "weight_ih_l") || !strcmp(rest, "weight_hh_l") || !strcmp(rest, "bias_ih_l") || !strcmp(rest, "bias_hh_l"));
    else
        ok = k == "gru.fc_output_layer.weight" || k == "gru.fc_output_layer.bias" || k == "gru.norm.weight" || k == "gru.norm.bias";
    if (!ok) return fail(e, SE_ERR_KEY, "unknown parameter key %s", key);
    e->weights_ready = false;
    return store_param(e, k, host_data, shape, ndim);
}

// (Re)allocates state for `batch` streams if needed and zeroes it asynchronously on `st`.
static int reset_on_stream(se_engine *e, int batch, hipStream_t st) {
    if (!e || batch <= 0) return fail(e, SE_ERR_ARG, "batch must be positive");
    int rc = ensure_ready(e);
    if (rc) return rc;
    const int L = e->L, T = e->T, B = batch, H = e->H, D = e->D, F0 = e->F[0];
    e->B = B;
    e->Bact = B;
    for (int &v : e->bact_slot) v = B;
    // a few streams give the bottleneck GEMMs a few hundred rows: a 256 x 128 tile per workgroup leaves 12-36 workgroups
    // walking K = 2048 alone (124 us at B = 1); the skinny 32 x 32-tile fp32 kernel (K split over the waves) takes 24
    select_gemm_route(e);
    size_t spec_n = (size_t)B * (stft_feat_route(e) ? 1 : e->M) * T * F0 * 2;  // the fused front end keeps microphone 0's spectrum only
    if (!e->io_fuse_on && (rc = dev_alloc(e, e->maskspec, (size_t)B * T * F0 * 2))) return rc;
    for (int r = 0; r < kRing; r++)
        if ((rc = dev_alloc(e, e->spec[r], spec_n)) || (rc = dev_alloc(e, e->gru_in[r], (size_t)B * T * D))) return rc;
    for (int i = 0; i < e->npre; i++) {
        const size_t nf = (size_t)B * e->Ch[0] * T * F0;
        for (int p = 0; p < 2; p++) {
            if ((rc = dev_alloc(e, e->pin[i][p], nf))) return rc;
            HIPCHECK(e, hipMemsetAsync(e->pin[i][p].p, 0, nf * sizeof(float), st));
        }
        if ((rc = dev_alloc(e, e->pre_stats[i], (size_t)B * 2 * (e->lv[i].pre.grid_x + 1)))) return rc;
        if ((rc = dev_alloc(e, e->pre_g, nf)) || (rc = dev_alloc(e, e->pre_out, nf))) return rc;
    }
    const size_t fcND = (size_t)(e->Ch[L] + 7) / 8 * e->F[L] * 8;  // fc output columns on the plane GEMM route (channels in whole octets)
    if ((rc = dev_alloc(e, e->fc_out, (size_t)B * T * std::max<size_t>(D, fcND)))) return rc;
    if (e->gemm_p && (rc = dev_alloc(e, e->fc_stats, (size_t)B * T * ((fcND + kGemmPBN - 1) / kGemmPBN) * 2))) return rc;
    for (int r = 0; r < kRing; r++) {
        if ((rc = dev_alloc(e, e->gi0[r], (size_t)B * T * 3 * H))) return rc;
        for (int l = 0; l < e->NL; l++)
            if ((rc = dev_alloc(e, e->seqr[l][r], (size_t)B * T * H))) return rc;
    }
    for (int l = 1; l < e->NL; l++)
        if ((rc = dev_alloc(e, e->gil[l], (size_t)B * T * 3 * H))) return rc;
    if (e->gemm_p) {
        // (sized for the bf16 planes also when the fp16 pair is on: a later weight load may fail the range guard and switch the
        //  format back without a re-plan of the batch; strides and buffer ranges follow buffer_planes() at every launch)
        const size_t PLn = operand_planes(e->precision);
        for (int r = 0; r < kRing; r++) {
            if ((rc = dev_alloc(e, e->gruinP[r], (PLn * B * T * D + 1) / 2))) return rc;
            for (int l = 0; l < e->NL; l++)
                if ((rc = dev_alloc(e, e->seqP[l][r], (PLn * B * T * H + 1) / 2))) return rc;
        }
    }
    for (int l = 0; l < e->NL; l++)
        for (int p = 0; p < 2; p++) {
            if ((rc = dev_alloc(e, e->hbuf[l][p], (size_t)B * H))) return rc;
            HIPCHECK(e, hipMemsetAsync(e->hbuf[l][p].p, 0, (size_t)B * H * sizeof(float), st));
        }
    select_all_p(e);
    if ((rc = alloc_state_p(e, st))) return rc;
    for (int l = 0; l < 4; l++) e->hcur[l] = 0;
    e->parity = 0;
    e->slot = 0;
    return SE_OK;
}

int se_reset(se_engine *e, int batch) {
    int rc = reset_on_stream(e, batch, nullptr);
    if (rc) return rc;
    HIPCHECK(e, hipDeviceSynchronize());
    return SE_OK;
}

int se_reset_stream(se_engine *e, int stream_index, void *stream) {
    if (!e) return SE_ERR_ARG;
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "se_reset_stream before se_reset");
    if (stream_index < 0 || stream_index >= e->B) return fail(e, SE_ERR_ARG, "stream index %d outside the batch of %d", stream_index, e->B);
    HIPCHECK(e, hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // conv time buffers = the tail of the current ring slot (the next window reads it as history)
    return state_rows_of(e, ~0u, [&](float *live, DevBuf &, long words) {
        HIPCHECK(e, hipMemsetAsync(live + words * stream_index, 0, (size_t)words * sizeof(float), st));
        return 0;
    });
}

int se_forward(se_engine *e, const float *x, float *y, void *stream) {
    if (!e || !x || !y) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "se_forward before se_reset");
    int rc = ensure_ready(e);
    if (rc) return rc;
    const long F = e->F[0], T = e->T, M = e->M;
    return forward_dev(e, reinterpret_cast<const cf2 *>(x), M * F * T, F * T, 1, T, reinterpret_cast<cf2 *>(y), F * T, 1, T,
                       static_cast<hipStream_t>(stream));
}


int se_stft(se_engine *e, const float *seg, int n, float *spec, void *stream) {
    if (!e || !seg || !spec || n <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    HIPCHECK(e, hipSetDevice(e->device));
    const long F = e->F[0], T = e->T;
    return launch_stft(e, seg, e->K, 0, 1, 0, e->K, SigRows{}, n, reinterpret_cast<cf2 *>(spec), F * T, 1, T, static_cast<hipStream_t>(stream));
}

int se_istft(se_engine *e, const float *spec, int n, float *wav, void *stream) {
    if (!e || !spec || !wav || n <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    HIPCHECK(e, hipSetDevice(e->device));
    const long F = e->F[0], T = e->T;
    return launch_istft(e, reinterpret_cast<const cf2 *>(spec), F * T, 1, T, n, wav, e->K, static_cast<hipStream_t>(stream));
}

static int ensure_stage_streams(se_engine *e) {
    if (e->stage_ready) return 0;
    int least = 0, greatest = 0;
    HIPCHECK(e, hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (int k = 0; k < 3; k++)  // the recurrence is a chain of short dependent launches: its waves go first when a CU frees up
        HIPCHECK(e, hipStreamCreateWithPriority(&e->stage_stream[k], hipStreamNonBlocking, k == 2 ? greatest : least));
    for (int r = 0; r < kRing; r++) {
        HIPCHECK(e, hipEventCreateWithFlags(&e->ev_enc[r], hipEventDisableTiming));
        HIPCHECK(e, hipEventCreateWithFlags(&e->ev_gru[r], hipEventDisableTiming));
        HIPCHECK(e, hipEventCreateWithFlags(&e->ev_dec[r], hipEventDisableTiming));
    }
    HIPCHECK(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    HIPCHECK(e, hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    e->stage_ready = true;
    return 0;
}

static int step_dev(se_engine *e, const float *src, long strideB, long strideM, long off, long Lsrc, SigRows rows, float *wav_out, long wav_ld, hipStream_t st) {
    const long F = e->F[0], T = e->T, M = e->M;
    int rc;
    const int prev = e->slot, cur = (e->slot + 1) % kRing;
    cf2 *spec = reinterpret_cast<cf2 *>(e->spec[cur].p);
    cf2 *ms = reinterpret_cast<cf2 *>(e->maskspec.p);
    e->slot = cur;
    // the fused ends (io_fused.hip.h) where the route has them: the spectrum buffer then holds microphone 0 only
    const bool ffeat = stft_feat_route(e), fmask = e->io_fuse_on;
    const long sB = ffeat ? T * F : M * T * F;
    if (ffeat) rc = stage_stft_feat_p(e, cur, src, strideB, strideM, off, Lsrc, rows, spec, st);
    else rc = launch_stft(e, src, strideB, strideM, (int)M, off, Lsrc, rows, e->Bact * (int)M, spec, T * F, F, 1, st);
    if (rc) return rc;
    if ((rc = run_encoder(e, cur, prev, spec, sB, T * F, F, 1, st, ffeat))) return rc;
    if ((rc = stage_bottleneck(e, cur, st))) return rc;
    if (fmask) return run_decoder(e, cur, spec, sB, F, 1, nullptr, 0, 0, 0, st, wav_out, wav_ld);
    if ((rc = run_decoder(e, cur, spec, sB, F, 1, ms, T * F, F, 1, st))) return rc;
    return launch_istft(e, ms, T * F, F, 1, e->Bact, wav_out, wav_ld, st);
}

int se_step(se_engine *e, const float *wav_in, float *wav_out, void *stream) {
    if (!e || !wav_in || !wav_out) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "se_step before se_reset");
    int rc = ensure_ready(e);
    if (rc) return rc;
    return step_dev(e, wav_in, (long)e->M * e->K, e->K, 0, e->K, SigRows{}, wav_out, e->K, static_cast<hipStream_t>(stream));
}

// ---- per-stream state rows (state_rows.hip.h) of the streams a ChainPlan names: dir 0 save, 1 restore, 2 zero ----
static int chain_rows(se_engine *e, unsigned which, int dir, StreamRange r, hipStream_t st) {
    if (r.count <= 0) return 0;
    StateRowList rows;
    state_rows_of(e, which, [&](float *live, DevBuf &carry, long words) { rows.add(live, carry.p, words); return 0; });
    ProfScope ps(e, "k_state_rows", dir == 0 ? "state_save" : dir == 1 ? "state_restore" : "state_zero", 0, st);
    rows.launch(st, dir, r.streams, r.count);
    HIPCHECK(e, hipGetLastError());
    return 0;
}

// the streams whose LAST segment is n keep what the stage(s) in `which` have just left behind
static int chain_save(se_engine *e, const ChainPlan *plan, long n, unsigned which, hipStream_t st) {
    return plan ? chain_rows(e, which, 0, plan->ending(n), st) : 0;
}

static int alloc_carry(se_engine *e) {
    return state_rows_of(e, ~0u, [&](float *, DevBuf &carry, long words) { return dev_alloc(e, carry, (size_t)e->B * words); });
}

// What run_segments walks: a uniform call's geometry (every stream: N segments from off_first, `skip` stripped), or a chains call's plan
// (chain_plan.h), which carries every stream's own length, first-segment offset and strip.
struct SegmentWalk {
    long N, off_first, skip;
    const ChainPlan *plan;
    SegmentWalk(const ChunkGeometry &g) : N(g.nseg), off_first(g.off0), skip(g.skip), plan(nullptr) {}
    SegmentWalk(const ChainPlan &p) : N(p.N), off_first(0), skip(0), plan(&p) {}
};

// The segments of one realtime_process call on state that is ready: w.N half-overlapping windows, window n of a stream starting at
// w.off_first + n * K/2 (+ the stream's own plan->off0), overlap-average with the strip taken off -> out [batch, length].
static int run_segments(se_engine *e, const float *mixture, int batch, int64_t length, const SegmentWalk &w, float *out, hipStream_t st);

int se_realtime_process(se_engine *e, const float *mixture, int batch, int64_t length, int flag, float *out, void *stream) {
    if (!e || !mixture || !out || batch <= 0 || length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    int rc;
    if (!flag) {
        if ((rc = reset_on_stream(e, batch, static_cast<hipStream_t>(stream)))) return rc;  // CRN.py:574-575
    } else {
        if (e->B != batch) return fail(e, SE_ERR_STATE, "flag=True with batch %d but the carried state holds %d streams", batch, e->B);
        if ((rc = ensure_ready(e))) return rc;
    }
    return run_segments(e, mixture, batch, length, chunk_geometry(e->K, length, flag), out, static_cast<hipStream_t>(stream));
}

int se_chunk_geometry(int segment_length, int64_t length, int continues, int64_t *nseg, int64_t *off0, int64_t *skip) {
    if (segment_length <= 0 || length <= 0 || !nseg || !off0 || !skip) return SE_ERR_ARG;
    const ChunkGeometry g = chunk_geometry(segment_length, length, continues != 0);
    *nseg = g.nseg; *off0 = g.off0; *skip = g.skip;
    return SE_OK;
}

static int run_segments(se_engine *e, const float *mixture, int batch, int64_t length, const SegmentWalk &w, float *out, hipStream_t st) {
    int rc;
    const long K = e->K, P = K / 2, Nseg = w.N, off_first = w.off_first;
    const ChainPlan *plan = w.plan;
    const SigRows rows = plan ? SigRows{plan->len, plan->off0} : SigRows{};
    if ((rc = dev_alloc(e, e->yseg, (size_t)batch * Nseg * K))) return rc;
    bool piped = e->pipeline && !e->prof_on && Nseg > 1;
    if (piped && ensure_stage_streams(e)) {  // no extra streams / events available: fall back to the caller's stream for good
        e->pipeline = 0;
        piped = false;
    }
    // launch batch of segment n: the prefix of streams still running when the plan is compact (see se_engine::Bact)
    static const bool compact_env = [] { const char *v = getenv("SE_RAGGED_COMPACT"); return !(v && v[0] == '0'); }();
    const bool compact = compact_env && plan && e->gemm_p && e->variant == 0;
    auto bact_of = [&](long n) { return compact ? plan->bact(n) : e->B; };
    struct RestoreBact {  // a failing call leaves the engine usable: nothing of the plan outlives the call
        se_engine *e;
        ~RestoreBact() { e->Bact = e->B; for (int &v : e->bact_slot) v = e->B; }
    } restore_bact{e};
    if (!piped) {
        for (long n = 0; n < Nseg; n++) {
            const long off = off_first + n * P;
            e->Bact = bact_of(n);
            // yseg is [B][Nseg][K]: the iSTFT writes segment n of every stream with row stride Nseg*K
            if ((rc = step_dev(e, mixture, (long)e->M * length, length, off, length, rows, e->yseg.p + n * K, Nseg * K, st))) return rc;
            if ((rc = chain_save(e, plan, n, ~0u, st))) return rc;
        }
    } else {
        // Segments are sequentially dependent only WITHIN a stage (conv history, GRU state), so the three stages run as a
        // software pipeline over segments on three streams: while the bottleneck of segment n walks its 2 x T dependent
        // GRU launches, the encoder of n+1.. and the decoder of n-1 keep the matrix cores and HBM busy.
        hipStream_t sE = e->stage_stream[0], sD = e->stage_stream[1], sG = e->stage_stream[2];
        const long F = e->F[0], T = e->T, M = e->M;
        const bool ffeat = stft_feat_route(e), fmask = e->io_fuse_on;  // the fused ends (io_fused.hip.h): one launch per segment each
        const long Ms = ffeat ? 1 : M;                                 // microphones in the staged spectra
        const size_t spec_n = (size_t)e->B * Ms * T * F * 2, mask_n = (size_t)e->B * T * F * 2;
        // The STFT of kFftSub segments is one launch on the encoder stream ahead of their encoders, the iSTFT one launch on
        // the decoder stream behind their decoders: both overlap with the other stages of neighbouring segments.
        const long CH = std::min<long>(Nseg, kPipeChunk);
        if ((rc = dev_alloc(e, e->spec_all, spec_n * CH)) || (!fmask && (rc = dev_alloc(e, e->mask_all, mask_n * CH)))) return rc;
        // layer l of a recurrence round works on segment (round - l); SE_GRU_DIRECT=0 pins the LDS-slice step kernel, which has
        // no multi-layer form: layers then run back to back
        const bool lagged = e->gru_direct != 0;
        const int NL = e->NL, lag = lagged ? NL - 1 : 0;
        for (long c0 = 0; c0 < Nseg; c0 += CH) {
            const long cn = std::min(CH, Nseg - c0);
            HIPCHECK(e, hipEventRecord(e->ev_fork, st));
            for (hipStream_t q : e->stage_stream) HIPCHECK(e, hipStreamWaitEvent(q, e->ev_fork, 0));
            const int slot0 = e->slot;  // segment i of this chunk lives in ring slot (slot0 + 1 + i) % kRing
            auto slot_of = [&](long i) { return (int)((slot0 + 1 + i) % kRing); };
            for (long i = 0; i < cn + lag; i++) {
                if (i < cn) {  // ---- encoder stream: STFT batch, features + encoder, GRU input projection of segment i ----
                    const int cur = slot_of(i), prev = slot_of(i - 1);
                    e->slot = cur;
                    e->Bact = e->bact_slot[cur] = bact_of(c0 + i);
                    const cf2 *spec = reinterpret_cast<const cf2 *>(e->spec_all.p + spec_n * i);
                    if (!ffeat && i % kFftSub == 0) {
                        const long ns = std::min<long>(kFftSub, cn - i);
                        if ((rc = launch_stft(e, mixture, (long)e->M * length, length, (int)M, off_first + (c0 + i) * P, length, rows, e->Bact * (int)M,
                                              reinterpret_cast<cf2 *>(e->spec_all.p + spec_n * i), T * F, F, 1, sE, (int)ns, P, (long)(spec_n / 2)))) return rc;
                    }
                    if (i >= kRing) HIPCHECK(e, hipStreamWaitEvent(sE, e->ev_dec[cur], 0));  // slot cur was last read by the decoder of segment i - kRing
                    // (the fused front end writes ring slot cur: it runs here, behind the slot's last reader, not kFftSub segments ahead)
                    if (ffeat && (rc = stage_stft_feat_p(e, cur, mixture, (long)e->M * length, length, off_first + (c0 + i) * P, length, rows,
                                                         reinterpret_cast<cf2 *>(e->spec_all.p + spec_n * i), sE))) return rc;
                    if ((rc = run_encoder(e, cur, prev, spec, Ms * T * F, T * F, F, 1, sE, ffeat))) return rc;
                    if ((rc = stage_gru_proj0(e, cur, sE))) return rc;
                    if ((rc = chain_save(e, plan, c0 + i, 1u, sE))) return rc;  // before the encoder stream reuses the slot, kRing segments on
                    HIPCHECK(e, hipEventRecord(e->ev_enc[cur], sE));
                    HIPCHECK(e, hipStreamWaitEvent(sG, e->ev_enc[cur], 0));
                }
                // ---- recurrence stream ----
                long done = -1;  // segment whose last layer completes in this round
                if (lagged) {
                    int slots[4] = {-1, -1, -1, -1};
                    for (int l = 0; l < NL; l++)
                        if (i - l >= 0 && i - l < cn) slots[l] = slot_of(i - l);
                    if ((rc = stage_gru_round(e, slots, sG))) return rc;
                    for (int l = 0; l < NL; l++)  // layer l has just finished segment i - l
                        if (slots[l] >= 0 && (rc = chain_save(e, plan, c0 + i - l, 2u << l, sG))) return rc;
                    done = i - (NL - 1);
                } else {
                    e->Bact = e->bact_slot[slot_of(i)];
                    for (int l = 0; l < NL; l++)
                        if ((rc = stage_gru_layer(e, l, slot_of(i), sG, /*overlapped=*/true))) return rc;
                    if ((rc = chain_save(e, plan, c0 + i, ~1u, sG))) return rc;
                    done = i;
                }
                if (done < 0 || done >= cn) continue;
                // ---- decoder stream: fc + norm, decoder, mask, iSTFT batch of segment `done` ----
                const int dcur = slot_of(done);
                e->Bact = e->bact_slot[dcur];
                HIPCHECK(e, hipEventRecord(e->ev_gru[dcur], sG));
                HIPCHECK(e, hipStreamWaitEvent(sD, e->ev_gru[dcur], 0));
                const cf2 *dspec = reinterpret_cast<const cf2 *>(e->spec_all.p + spec_n * done);
                cf2 *ms = fmask ? nullptr : reinterpret_cast<cf2 *>(e->mask_all.p + mask_n * done);
                if ((rc = stage_gru_out(e, dcur, sD))) return rc;
                // (the fused back end reads the single dec3 buffer: it runs per segment, inside the decoder stage, before ev_dec)
                if (fmask) rc = run_decoder(e, dcur, dspec, Ms * T * F, F, 1, nullptr, 0, 0, 0, sD, e->yseg.p + (c0 + done) * K, Nseg * K);
                else rc = run_decoder(e, dcur, dspec, Ms * T * F, F, 1, ms, T * F, F, 1, sD);
                if (rc) return rc;
                if (!fmask && (done % kFftSub == kFftSub - 1 || done == cn - 1)) {
                    const long i0 = done - done % kFftSub;
                    if ((rc = launch_istft(e, reinterpret_cast<const cf2 *>(e->mask_all.p + mask_n * i0), T * F, F, 1, bact_of(c0 + i0) /* (the ring slot of segment i0 has been reused by now) */,
                                           e->yseg.p + (c0 + i0) * K, Nseg * K, sD, (int)(done - i0 + 1), (long)(mask_n / 2), K))) return rc;
                }
                HIPCHECK(e, hipEventRecord(e->ev_dec[dcur], sD));
            }
            for (hipStream_t q : e->stage_stream) {  // the last decoder implies every earlier stage, but the join costs nothing
                HIPCHECK(e, hipEventRecord(e->ev_join, q));
                HIPCHECK(e, hipStreamWaitEvent(st, e->ev_join, 0));
            }
        }
    }
    // the streams that ended before the longest one get their own state back (the stage streams have joined `st`)
    if (plan && (rc = chain_rows(e, ~0u, 1, plan->ended_early(), st))) return rc;
    launch_k_overlap_avg(dim3((unsigned)((length + 255) / 256), batch), st, e->yseg.p, out, (int)Nseg, (int)K, (long)length, w.skip, rows.len,
                         plan ? plan->skip : nullptr);
    HIPCHECK(e, hipGetLastError());
    return SE_OK;
}

// A batch of chunk chains (include/se_engine.h): reset or make ready, plan (chain_plan.h), upload, zero the flag-0 rows, run
int se_realtime_process_chains(se_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host,
                               const uint8_t *flags_host, float *out, void *stream) {
    if (!e || !mixture || !out || !lengths_host || !flags_host || batch <= 0 || max_length <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    ChainPlan plan;
    std::string err;
    int uniform_flag = 0;
    int rc = plan_chains(plan, e->K, batch, max_length, lengths_host, flags_host, e->B, &uniform_flag, err);
    if (rc == kPlanUniform) return se_realtime_process(e, mixture, batch, max_length, uniform_flag, out, stream);
    if (rc) return fail(e, rc, "%s", err.c_str());
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = plan.continues() ? ensure_ready(e) : reset_on_stream(e, batch, st))) return rc;
    if ((rc = alloc_carry(e)) || (rc = upload_plan(e, e->plan_dev, plan, st))) return rc;
    // a reset among continuing streams: zero those streams' rows (se_reset_stream for any number of streams in one launch)
    if (plan.continues() && (rc = chain_rows(e, ~0u, 2, plan.reset_streams(), st))) return rc;
    return run_segments(e, mixture, batch, max_length, plan, out, st);
}

// a chains call in which every stream has the one flag
int se_realtime_process_ragged(se_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host, int flag, float *out,
                               void *stream) {
    if (batch <= 0) return fail(e, SE_ERR_ARG, "bad argument");
    const std::vector<uint8_t> flags((size_t)batch, flag ? 1 : 0);
    return se_realtime_process_chains(e, mixture, batch, max_length, lengths_host, flags.data(), out, stream);
}

static int copy_out(se_engine *e, const float *dev, size_t n, float *host, int64_t cap, int64_t *count, hipStream_t st) {
    if (count) *count = (int64_t)n;
    if ((int64_t)n > cap) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
    HIPCHECK(e, hipStreamSynchronize(st));
    HIPCHECK(e, hipMemcpy(host, dev, n * sizeof(float), hipMemcpyDeviceToHost));
    return SE_OK;
}

static int read_tap_impl(se_engine *e, const char *name, float *host_out, float *dev_out, int64_t capacity, int64_t *count, void *stream);

int se_read_tap(se_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream) {
    if (!e || !name || !host_out) return fail(e, SE_ERR_ARG, "null argument");
    return read_tap_impl(e, name, host_out, nullptr, capacity, count, stream);
}

// The distillation feature maps "ft0".."ft<L>" straight into DEVICE memory ([B, C, F, T] fp32), enqueued on `stream`, no host copy and no
// synchronisation: what a distillation training loop consumes (distillation_crn.py:467-477).  Other taps are host-only (se_read_tap).
int se_read_tap_dev(se_engine *e, const char *name, float *dev_out, int64_t capacity, int64_t *count, void *stream) {
    if (!e || !name || !dev_out) return fail(e, SE_ERR_ARG, "null argument");
    if (strncmp(name, "ft", 2)) return fail(e, SE_ERR_KEY, "se_read_tap_dev serves the feature taps ft0..ft%d only (got %s)", e->L, name);
    return read_tap_impl(e, name, nullptr, dev_out, capacity, count, stream);
}

static int read_tap_impl(se_engine *e, const char *name, float *host_out, float *dev_out, int64_t capacity, int64_t *count, void *stream) {
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no forward has run");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int L = e->L, T = e->T, B = e->B, cur = e->slot;
    int C = 0, F = 0, idx = -1;
    if (host_out && !strcmp(name, "gemm_kblock")) {  // one value, no tensor: 1 where this batch's bottleneck GEMMs run on K-blocked operands
        if (count) *count = 1;
        if (capacity < 1) return fail(e, SE_ERR_ARG, "buffer too small: need 1 float");
        host_out[0] = e->gemm_p && kblock_on(e) ? 1.0f : 0.0f;
        return SE_OK;
    }
    if (strncmp(name, "ft", 2)) {  // operand tensors are split-bf16 planes, summed back on the host
        se_convp_state &S = *e->cp;
        const float *psrc = nullptr;
        PlaneBuf kind = PlaneBuf::kConvAct;
        if (!strcmp(name, "feat")) { kind = PlaneBuf::kFeature; psrc = S.xinP[0].p + (size_t)cur * S.slot_elems[0] * 4; C = e->Ch[0]; F = e->F[0]; }
        else if (!strcmp(name, "gru")) { psrc = S.decinP[cur].p; C = e->Ch[L]; F = e->F[L]; }
        else if (sscanf(name, "enc%d", &idx) == 1 && idx >= 0 && idx < L - 1) { psrc = S.xinP[idx + 1].p + (size_t)cur * S.slot_elems[idx + 1] * 4; C = e->Ch[idx + 1]; F = e->F[idx + 1]; }
        else if (sscanf(name, "dec%d", &idx) == 1 && idx >= 0 && idx < L - 1) { psrc = S.decP[idx].p; C = e->Ch[L - 1 - idx]; F = e->F[L - 1 - idx]; }
        if (psrc) {
            const size_t n = (size_t)B * C * T * F;
            if (count) *count = (int64_t)n;
            if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
            return p_to_host(e, psrc, kind, C, F, host_out, st, true);
        }
        if (sscanf(name, "enc%d", &idx) != 1 || idx != L - 1) return fail(e, SE_ERR_KEY, "unknown tap %s", name);
        // the GRU input: GEMM A planes [PL][B*T][(o*F+f)*8+c] (k_gemm_p) or fp32 rows [B][T][C*F]
        const int Cl = e->Ch[L], Fl = e->F[L], PLn = buffer_planes(e->precision, e->pair_on, PlaneBuf::kGemmA), D = e->D;
        const bool pair = buffer_format(e->precision, e->pair_on, PlaneBuf::kGemmA) == PlaneFmt::kF16Pair;
        const size_t n = (size_t)B * Cl * T * Fl;
        if (count) *count = (int64_t)n;
        if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
        HIPCHECK(e, hipStreamSynchronize(st));
        if (!e->gemm_p) {
            std::vector<float> h(n);
            HIPCHECK(e, hipMemcpy(h.data(), e->gru_in[cur].p, n * sizeof(float), hipMemcpyDeviceToHost));
            for (int b = 0; b < B; b++)
                for (int c = 0; c < Cl; c++)
                    for (int t = 0; t < T; t++)
                        for (int f = 0; f < Fl; f++) host_out[(((size_t)b * Cl + c) * Fl + f) * T + t] = h[(((size_t)b * T + t) * Cl + c) * Fl + f];
            return SE_OK;
        }
        std::vector<uint16_t> h((size_t)PLn * B * T * D);
        HIPCHECK(e, hipMemcpy(h.data(), e->gruinP[cur].p, h.size() * 2, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; b++)
            for (int c = 0; c < Cl; c++)
                for (int t = 0; t < T; t++)
                    for (int f = 0; f < Fl; f++) {
                        float v = 0;
                        uint16_t up[3] = {0, 0, 0};
                        for (int pl = 0; pl < PLn; pl++) {
                            const size_t row = (size_t)b * T + t, k = ((size_t)(c >> 3) * Fl + f) * 8 + (c & 7);
                            const uint16_t u = kblock_on(e) ? h[kblock_index((long)row, D, (long)k, pl)] : h[((size_t)pl * B * T + row) * D + k];
                            up[pl] = u;
                            if (PLn == 1) { _Float16 hv; memcpy(&hv, &u, 2); v += (float)hv; } else v += bf16_to_f32(u);
                        }
                        if (pair) v = join2h(up[0], up[1]);
                        host_out[(((size_t)b * Cl + c) * Fl + f) * T + t] = v;
                    }
        return SE_OK;
    }
    if (sscanf(name, "ft%d", &idx) == 1 && idx >= 0 && idx <= L) {
        // Pre-activation feature maps of the distillation student (distillation_crn.py:222-228, 126-128, 262-264, 467-477):
        // ft0 = last encoder block's convolution output, ft1 = fc_output_layer output ([B, T, D] memory viewed as [B, C, F, T],
        // distillation_crn.py:364), ft2.. = transposed-convolution outputs of decoder blocks 0..L-2 (before activation, norm and
        // frequency padding).  The hot path fuses the activation into the producing kernel, so the tap RE-RUNS that one launch
        // (launch_enc_conv_p / launch_dec_conv_p, as the stage makes it) without activation and statistics on the planes still held
        // in the ring slot, into a scratch buffer in the R layout; k_tap_r_to_bcft transposes it.  Nothing on the inference path
        // pays for it.  ft1 is one GEMM on the last layer's sequence.
        const int prev = (cur + kRing - 1) % kRing;
        int rc = ensure_ready(e);
        if (rc) return rc;
        se_convp_state &S = *e->cp;
        struct AllStreams {  // launch_conv_p covers Bact streams: the tap covers the allocation batch
            se_engine *e; int keep;
            ~AllStreams() { e->Bact = keep; }
        } all_streams{e, e->Bact};
        e->Bact = B;
        struct Scratch {
            DevBuf r, t;  // the re-run's output; the transposed map of the host form
            ~Scratch() { dev_free(r); dev_free(t); }
        } tmp;
        // oT / Fh: the R layout's positions (k_tap_r_to_bcft); oT = 0: tmp.r already holds [B, T, D] = [B, C, F, T] memory (ft1)
        auto finish = [&](int C_, int F_, int oT, int Fh) -> int {
            const size_t n_ = (size_t)B * C_ * T * F_;
            if (count) *count = (int64_t)n_;
            if ((int64_t)n_ > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n_);
            // device form: one transposition (or copy) into dev_out; host form: the same launch into tmp.t, then a copy
            const float *map = tmp.r.p;
            if (oT) {
                if (!dev_out && (rc = dev_alloc(e, tmp.t, n_))) return rc;
                float *dst = dev_out ? dev_out : tmp.t.p;
                hipLaunchKernelGGL(k_tap_r_to_bcft, dim3(1024), dim3(256), 0, st, tmp.r.p, dst, B, C_, T, F_, oT, Fh);
                HIPCHECK(e, hipGetLastError());
                map = dst;
            } else if (dev_out) HIPCHECK(e, hipMemcpyAsync(dev_out, map, n_ * sizeof(float), hipMemcpyDeviceToDevice, st));
            HIPCHECK(e, hipStreamSynchronize(st));  // the scratch is freed on return (the re-run itself is the expensive part)
            if (host_out) HIPCHECK(e, hipMemcpy(host_out, map, n_ * sizeof(float), hipMemcpyDeviceToHost));
            return SE_OK;
        };
        if (idx == 0) {
            const int i = L - 1, Co = e->Ch[L], Fo = e->F[L];
            const ConvPPlan *pl;
            if ((rc = tap_enc_plan(e, &pl)) || (rc = dev_alloc(e, tmp.r, (size_t)B * pl->a.y_stream))) return rc;
            if ((rc = launch_enc_conv_p(e, i, *pl, cur, prev, tmp.r.p, nullptr, nullptr, false, st, "tap_ft"))) return rc;
            return finish(Co, Fo, Fo, 0);
        }
        if (idx == 1) {
            const int D = e->D, H = e->H;
            if ((rc = dev_alloc(e, tmp.r, (size_t)B * T * D))) return rc;
            if ((rc = launch_gemm(e, e->seqr[e->NL - 1][cur].p, H, e->fcw.p, H, e->fcb.p, tmp.r.p, D, B * T, D, H, 0, st, "tap_ft", e->fcw_x.p))) return rc;
            return finish(e->Ch[L], e->F[L], 0, 0);
        }
        const int j = idx - 2, lvl = L - 1 - j;
        if (lvl <= 0) return fail(e, SE_ERR_KEY, "unknown tap %s", name);
        const int Co = e->Ch[lvl], Fi = e->F[lvl + 1];
        if ((rc = dev_alloc(e, tmp.r, (size_t)B * S.pv[j].dec_even.a.y_stream))) return rc;
        const float *xin = j == 0 ? S.decinP[cur].p : S.decP[j - 1].p;
        if ((rc = launch_dec_conv_p(e, j, reinterpret_cast<const uint4 *>(xin), tmp.r.p, nullptr, false, st, "tap_ft"))) return rc;
        return finish(Co, 2 * Fi - 1, 2 * Fi, Fi);
    }
    return fail(e, SE_ERR_KEY, "unknown tap %s", name);
}

int se_export_state(se_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream) {
    if (!e || !name || !host_out) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no state: call se_reset first");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = e->B, T = e->T, H = e->H;
    int idx = -1;
    if (!strcmp(name, "h")) {
        const size_t n = (size_t)e->NL * B * H;
        if (count) *count = (int64_t)n;
        if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
        HIPCHECK(e, hipStreamSynchronize(st));
        for (int l = 0; l < e->NL; l++)
            HIPCHECK(e, hipMemcpy(host_out + (size_t)l * B * H, e->hbuf[l][e->hcur[l]].p, (size_t)B * H * sizeof(float), hipMemcpyDeviceToHost));
        return SE_OK;
    }
    const bool is_pbuf = sscanf(name, "pbuf%d", &idx) == 1 && idx >= 0 && idx < e->npre;
    if (is_pbuf || (sscanf(name, "buf%d", &idx) == 1 && idx >= 0 && idx < e->L)) {
        const int C = is_pbuf ? e->Ch[0] : e->Ch[idx], F = is_pbuf ? e->F[0] : e->F[idx], P = is_pbuf ? 4 : (2 << idx);
        const size_t n = (size_t)B * C * F * P, nsrc = (size_t)B * C * T * F;
        if (count) *count = (int64_t)n;
        if ((int64_t)n > capacity) return fail(e, SE_ERR_ARG, "buffer too small: need %zu floats", n);
        std::vector<float> h(nsrc);
        HIPCHECK(e, hipStreamSynchronize(st));
        if (!is_pbuf) {
            int rc = p_to_host(e, e->cp->xinP[idx].p + (size_t)e->slot * e->cp->slot_elems[idx] * 4, xin_kind(idx), C, F, h.data(), st, false);
            if (rc) return rc;
        } else if (e->cp->pre_p) {
            int rc = p_to_host(e, e->cp->pinP[idx].p + (size_t)e->slot * e->cp->pslot_elems * 4, PlaneBuf::kFeature, C, F, h.data(), st, false);
            if (rc) return rc;
        } else
        HIPCHECK(e, hipMemcpy(h.data(), e->pin[idx][e->parity].p, nsrc * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t bc = 0; bc < (size_t)B * C; bc++)
            for (int f = 0; f < F; f++)
                for (int p = 0; p < P; p++) host_out[(bc * F + f) * P + p] = h[(bc * T + (T - P + p)) * F + f];
        return SE_OK;
    }
    return fail(e, SE_ERR_KEY, "unknown state %s", name);
}

int se_import_state(se_engine *e, const char *name, const float *host_in, int64_t count, void *stream) {
    if (!e || !name || !host_in) return fail(e, SE_ERR_ARG, "null argument");
    if (e->B <= 0) return fail(e, SE_ERR_STATE, "no state: call se_reset first");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = e->B, T = e->T, H = e->H;
    int idx = -1;
    HIPCHECK(e, hipStreamSynchronize(st));
    if (!strcmp(name, "h")) {
        if (count != (int64_t)e->NL * B * H) return fail(e, SE_ERR_SHAPE, "state h needs %d floats", e->NL * B * H);
        for (int l = 0; l < e->NL; l++)
            HIPCHECK(e, hipMemcpy(e->hbuf[l][e->hcur[l]].p, host_in + (size_t)l * B * H, (size_t)B * H * sizeof(float), hipMemcpyHostToDevice));
        return SE_OK;
    }
    const bool is_pbuf = sscanf(name, "pbuf%d", &idx) == 1 && idx >= 0 && idx < e->npre;
    if (is_pbuf || (sscanf(name, "buf%d", &idx) == 1 && idx >= 0 && idx < e->L)) {
        const int C = is_pbuf ? e->Ch[0] : e->Ch[idx], F = is_pbuf ? e->F[0] : e->F[idx], P = is_pbuf ? 4 : (2 << idx);
        if (count != (int64_t)B * C * F * P) return fail(e, SE_ERR_SHAPE, "state %s needs %ld floats", name, (long)B * C * F * P);
        const size_t nsrc = (size_t)B * C * T * F;
        std::vector<float> h(nsrc, 0.0f);
        for (size_t bc = 0; bc < (size_t)B * C; bc++)
            for (int f = 0; f < F; f++)
                for (int p = 0; p < P; p++) h[(bc * T + (T - P + p)) * F + f] = host_in[(bc * F + f) * P + p];
        if (!is_pbuf) return host_to_p(e, h, xin_kind(idx), C, F, e->cp->xinP[idx].p + (size_t)e->slot * e->cp->slot_elems[idx] * 4);
        if (e->cp->pre_p) return host_to_p(e, h, PlaneBuf::kFeature, C, F, e->cp->pinP[idx].p + (size_t)e->slot * e->cp->pslot_elems * 4);
        HIPCHECK(e, hipMemcpy(e->pin[idx][e->parity].p, h.data(), nsrc * sizeof(float), hipMemcpyHostToDevice));
        return SE_OK;
    }
    return fail(e, SE_ERR_KEY, "unknown state %s", name);
}

double se_flops_per_frame(const se_engine *e) {
    if (!e) return 0;
    const int L = e->L, T = e->T, H = e->H, D = e->D;
    double mac = 0;
    for (int i = 0; i < L; i++) mac += (double)e->Ch[i + 1] * e->Ch[i] * 15 * e->F[i + 1] * T;
    if (e->variant) {
        for (int i = 0; i < L; i++) mac += 2.0 * e->Ch[i + 1] * e->Ch[i + 1] * e->F[i + 1] * T;  // conv_trans + conv_gated
        mac += 3.0 * ((double)e->Ch[0] * e->Ch[0] * 25 + 2.0 * e->Ch[0] * e->Ch[0]) * e->F[0] * T;  // preconv blocks
    }
    for (int j = 0; j < L; j++) {
        const int lvl = L - 1 - j, Ci = e->Ch[lvl + 1], Co = lvl == 0 ? 2 : e->Ch[lvl];
        mac += (double)Ci * Co * 15 * e->F[lvl + 1] * T;
        if (lvl > 0) mac += 2.0 * Co * Co * e->F[lvl] * T;
    }
    for (int l = 0; l < e->NL; l++) mac += (double)T * (3.0 * H * (l == 0 ? D : H) + 3.0 * H * H);
    mac += (double)T * D * H;
    return 2.0 * mac;
}

int se_frames_per_segment(const se_engine *e) { return e ? e->T : 0; }

int se_profile(se_engine *e, int enable) {
    if (!e) return SE_ERR_ARG;
    HIPCHECK(e, hipSetDevice(e->device));
    HIPCHECK(e, hipDeviceSynchronize());
    for (auto &r : e->prof_recs) { e->prof_pool.push_back(r.a); e->prof_pool.push_back(r.b); }
    e->prof_recs.clear();
    for (auto &l : e->prof_labels) { l.ms = 0; l.launches = 0; }
    e->prof_on = enable != 0;
    return SE_OK;
}

int se_profile_read(se_engine *e, int index, char *kernel, char *label, int cap, double *ms_total, int64_t *launches, double *flops_per_launch) {
    if (!e) return SE_ERR_ARG;
    if (!e->prof_recs.empty()) {  // fold pending records
        HIPCHECK(e, hipDeviceSynchronize());
        for (auto &r : e->prof_recs) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { e->prof_labels[r.label].ms += ms; e->prof_labels[r.label].launches++; }
            e->prof_pool.push_back(r.a); e->prof_pool.push_back(r.b);
        }
        e->prof_recs.clear();
    }
    if (index < 0 || index >= (int)e->prof_labels.size()) return 1;  // end of list
    const auto &l = e->prof_labels[index];
    if (kernel) snprintf(kernel, cap, "%s", l.kernel.c_str());
    if (label) snprintf(label, cap, "%s", l.label.c_str());
    if (ms_total) *ms_total = l.ms;
    if (launches) *launches = l.launches;
    if (flops_per_launch) *flops_per_launch = l.flops;
    return SE_OK;
}

}  // extern "C"

#include "fsn_engine.inc.h"
#include "train_ops.inc.h"
#include "fsn_train.inc.h"
