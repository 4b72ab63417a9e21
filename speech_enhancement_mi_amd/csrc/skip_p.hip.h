// skip_p.hip.h - the decoder's skip gate as ONE streaming kernel per level (reference CRN.py:387-396):
//
//     m   = sigmoid(gLN(residualmask(res)))          1x1 conv of the encoder output `res`, per-stream global layer norm
//     out = m * act(residual(res)) + (1 - m) * pad(gLN(act(deconv)))
//
// The global layer norm of the residualmask output needs that convolution's per-stream statistics BEFORE any output can be
// gated.  The first form of the plane path ran a statistics-only k_conv_p launch followed by a second k_conv_p launch with
// the gate in its epilogue: two LDS-staged launches of a few MFMAs each, 7.5 rounds of workgroups whose DMA latency,
// barriers and fragment fetches were all exposed (100 us per level for 13 us of memory traffic).  A 1x1 convolution has no
// halo and (with <= 32 output rows per M tile) nothing to share through LDS, so here ONE workgroup owns one stream and
// streams it twice through registers:
//     pass 1   B fragments straight from the P layout (16-byte pieces, consecutive lanes = consecutive positions),
//              residualmask rows only -> (sum, sum of squares) -> workgroup reduction -> mean / inverse deviation
//     pass 2   the same fragments again (L2 / MALL hits), residualmask + residual rows -> gate -> P layout of the block output
// Weights (<= 48 KB) sit in LDS in fragment order; no barrier inside either pass.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_p.hip.h"

namespace se {

// one 32-row M tile `mt` of the 1x1 convolutions on the B fragments of one position tile (K steps x planes), weights from LDS
template <int PL, int KP, PlaneFmt FMT, int APL>
__device__ __forceinline__ f32x16 skip_mma_tile(const uint4 *wl, int mt, const uint4 (&bf)[KP][APL], int l31, int half) {
    constexpr bool PAIR = FMT == PlaneFmt::kF16Pair;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; r++) c[r] = 0.0f;
#pragma unroll
    for (int kp = 0; kp < KP; kp++) {
        const uint4 *wf = wl + ((long)(mt * KP + kp) * PL) * 64 + l31 * 2 + half;
        if constexpr (PAIR) {
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            const h8 bh = __builtin_bit_cast(h8, bf[kp][0]), bl = __builtin_bit_cast(h8, bf[kp][APL > 1 ? 1 : 0]);
            uint4 w0, w1, w2;
            if constexpr (PL == kPairPlanesW2) { w1 = wf[0]; w2 = wf[64]; w0 = pair_scale_hi(w2); }
            else { w0 = wf[0]; w1 = wf[PL > 1 ? 64 : 0]; w2 = wf[PL > 2 ? 128 : 0]; }
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, w0), bh, c, 0, 0, 0);  // 2^11 w_hi * x_hi
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, w1), bh, c, 0, 0, 0);  // w_lo * x_hi
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, w2), bl, c, 0, 0, 0);  // w_hi * x_lo
        } else if (PL >= 2) {
            const bf16x8 a0 = __builtin_bit_cast(bf16x8, wf[0]), a1 = __builtin_bit_cast(bf16x8, wf[PL > 1 ? 64 : 0]);
            const bf16x8 b0 = __builtin_bit_cast(bf16x8, bf[kp][0]), b1 = __builtin_bit_cast(bf16x8, bf[kp][PL > 1 ? 1 : 0]);
            if (PL == 3) {
                const bf16x8 a2 = __builtin_bit_cast(bf16x8, wf[PL > 2 ? 128 : 0]), b2 = __builtin_bit_cast(bf16x8, bf[kp][PL > 2 ? 2 : 0]);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c, 0, 0, 0);
            }
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c, 0, 0, 0);
        } else {
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, wf[0]), __builtin_bit_cast(h8, bf[kp][0]), c, 0, 0, 0);
        }
    }
    if constexpr (PAIR) {
#pragma unroll
        for (int r = 0; r < 16; r++) c[r] *= kPairInvScale;
    }
    return c;
}

// Per-channel constants in LDS, one row of 8 floats per (octet, constant): cst[(oct * kSkipCst + k) * 8 + q], channel oct * 8 + q.
// A lane reads the 8 channels of one constant as two 16-byte pieces, once per (tile, octet).  Padded channels hold zeros.
enum SkipCst : int { kCstMaskB = 0, kCstResB = 1, kCstNormW = 2, kCstNormB = 3, kCstMaskNormW = 4, kCstMaskNormB = 5, kSkipCst = 6 };

__device__ __forceinline__ void skip_cst8(const float *cst, int oct, int k, float (&v)[8]) {
    const float4 *src = reinterpret_cast<const float4 *>(cst) + (oct * kSkipCst + k) * 2;
    const float4 u0 = src[0], u1 = src[1];
    v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
}

// kSkipFastGate: the gate of k_skip_p / k_skip_pd on subtract-then-FMA norms and the hardware exp2 / rcp (other bits than the
// kPOutBlend epilogue of k_conv_p, which keeps the expression below and is the reference of tests/test_gpu_skip_gate.py).  The workgroup
// then rewrites three constant rows once the mask statistics are known (skip_fold_stats): kCstMaskB = mu - bias, kCstMaskNormW =
// iu * weight, kCstNormW = iy * weight.  The means stay subtractions: folded into the additive constant they cost 3-30x in gate
// error at mean / sigma >= 10 (tests/test_skip_gate_cpu.py).
// Not with two bf16 planes: the gate's output differs from the epilogue's by 2e-7 relative, which the fp16 pair and three bf16 planes
// carry and one fp16 plane (bars of 1e-4) does not see, while two bf16 planes round it up to 2-3e-6 at the model output, over the 2e-6
// between two routes.  That mode keeps the epilogue's expression, its contractions written out.
constexpr bool kSkipFastGate = true;
template <int PL, PlaneFmt FMT>
constexpr bool skip_fast_gate() { return kSkipFastGate && (FMT == PlaneFmt::kF16Pair || PL != 2); }

struct SkipNorm { float my, iy, mu, iu; };  // mean and inverse deviation of the deconvolution and of residualmask(res)

// (the four are the same in every lane: kept in scalar registers)
__device__ __forceinline__ void skip_norm_uniform(SkipNorm &n) {
    for (float *f : {&n.my, &n.iy, &n.mu, &n.iu}) *f = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, *f)));
}

template <bool FAST>
__device__ __forceinline__ void skip_fold_stats(float *cst, int Cp, int tid, int nthreads, const SkipNorm &n) {
    if constexpr (FAST) {
        for (int ch = tid; ch < Cp; ch += nthreads) {
            float *row = cst + (ch >> 3) * kSkipCst * 8 + (ch & 7);
            row[kCstMaskB * 8] = n.mu - row[kCstMaskB * 8];
            row[kCstMaskNormW * 8] = n.iu * row[kCstMaskNormW * 8];
            row[kCstNormW * 8] = n.iy * row[kCstNormW * 8];
        }
        __syncthreads();
    }
}

// The gate of one octet `oct` (8 channels) at one position: um / ur the residualmask / residual accumulators, yv the deconvolution
// values (has_y: the column exists, CRN.py:389-392), nv = C - 8 oct valid channels.  bias, activation, the two norms, sigmoid, blend.
template <int ACT, bool FAST>
__device__ __forceinline__ void skip_gate_octet(const float *cst, int oct, int nv, const float (&um)[8], const float (&ur)[8], const float (&yv)[8],
                                                bool has_y, const SkipNorm &n, float (&o)[8]) {
    static_assert(ACT == 1 || ACT == 2, "ReLU or ELU");
    // Two halves of 4 values, each in three steps (sigmoid; activation; norm and blend) with the 16-byte pieces of the constant rows
    // a step needs: 12 registers at the most, where all six rows of the octet would be 48.  The row index passes through
    // an empty asm together with a result of the step before, so that a step's LDS reads stay behind that step (and the first step's
    // behind the octet's MFMAs); the pieces pass through one so that they stay 16-byte reads and are not sunk into a branch on has_y.
    auto piece = [&](int h4, int k, float (&c)[4]) {
        const float4 u = reinterpret_cast<const float4 *>(cst)[(oct * kSkipCst + k) * 2 + h4];
        c[0] = u.x; c[1] = u.y; c[2] = u.z; c[3] = u.w;
        asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]));
    };
    float um0 = um[0];
    asm volatile("" : "+v"(oct), "+v"(um0));
#pragma unroll
    for (int h4 = 0; h4 < 2; h4++) {
        float g[4], ca[4], cb[4], cc[4];
        piece(h4, kCstMaskB, ca); piece(h4, kCstMaskNormW, cb); piece(h4, kCstMaskNormB, cc);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = h4 * 4 + j;
            if constexpr (FAST) {
                const float un = __builtin_fmaf((q ? um[q] : um0) - ca[j], cb[j], cc[j]);
                g[j] = __builtin_amdgcn_rcpf(1.0f + __expf(-un));  // exp overflows to inf for un < -88: rcp(inf) = 0
            } else {  // (the contraction written out: every instance of either kernel rounds alike, whatever surrounds the call)
#pragma clang fp contract(off)
                const float u = (q ? um[q] : um0) + ca[j];
                const float un = __builtin_fmaf((u - n.mu) * n.iu, cb[j], cc[j]);
                g[j] = 1.0f / (1.0f + expf(-un));
            }
        }
        asm volatile("" : "+v"(oct), "+v"(g[3]));
        float v[4];
        piece(h4, kCstResB, ca);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float r = ur[h4 * 4 + j] + ca[j];
            if constexpr (ACT == 1) v[j] = fmaxf(r, 0.0f);
            else v[j] = r > 0.0f ? r : expf(r) - 1.0f;
        }
        asm volatile("" : "+v"(oct), "+v"(v[3]));
        piece(h4, kCstNormW, cb); piece(h4, kCstNormB, cc);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = h4 * 4 + j;
            float res;
            if constexpr (FAST) {
                const float yn = has_y ? __builtin_fmaf(yv[q] - n.my, cb[j], cc[j]) : 0.0f;
                res = __builtin_fmaf(g[j], v[j] - yn, yn);
            } else {
#pragma clang fp contract(off)
                const float yn = has_y ? __builtin_fmaf((yv[q] - n.my) * n.iy, cb[j], cc[j]) : 0.0f;
                res = __builtin_fmaf(g[j], v[j], (1.0f - g[j]) * yn);
            }
            o[q] = q < nv ? res : 0.0f;
        }
        if (h4 == 0) asm volatile("" : "+v"(oct), "+v"(o[3]));
    }
}

// pass 1's share of one M tile: sum and sum of squares of residualmask(res) + bias over the 16 channels of this lane (padded channels
// have zero weight rows and a zero bias: they add exact zeros)
__device__ __forceinline__ void skip_stat_tile(const float *cst, int mt, int half, const f32x16 &c, float &ts, float &tq) {
#pragma unroll
    for (int hh = 0; hh < 2; hh++) {
        float bm[8];
        skip_cst8(cst, mt * 4 + 2 * half + hh, kCstMaskB, bm);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float v = c[hh * 8 + q] + bm[q];
            ts += v; tq = __builtin_fmaf(v, v, tq);
        }
    }
}

// NW = waves per workgroup: 16 (1024 threads, 128 VGPRs) for KP <= 2, 8 for KP = 4 - the kernel is a latency-bound stream
// (one workgroup per CU), so bytes in flight = waves x fragments in flight decide its rate
// FMT = kF16Pair (PL = 3 weight planes): res and out are two fp16 planes (split_f16pair.h), the weights (2^11 w_hi, w_lo, w_hi), three f16
// MFMAs per K step in the fixed order W0 b_hi, W1 b_hi, W2 b_lo, and the 2^-11 (exact) on the accumulators before the statistics of
// pass 1 and before the gate of pass 2.  PL = 2 with kF16Pair: the two stored planes (w_lo, w_hi) in LDS, 2^11 w_hi made when the
// fragment is read (pair_scale_hi) - the same operands from two thirds of the weight bytes.
template <int PL, int KP, int NW, int ACT, PlaneFmt FMT = PlaneFmt::kBf16>
__global__ __launch_bounds__(NW * 64) void k_skip_p(SkipPArgs a) {
    constexpr bool PAIR = FMT == PlaneFmt::kF16Pair;
    static_assert(!PAIR || PL == kPairPlanesW || PL == kPairPlanesW2, "the fp16 pair form has three weight planes, or two stored ones");
    constexpr int APL = PAIR ? kPairPlanesA : PL;  // planes of res and out
    extern __shared__ __align__(16) uint4 wl[];  // [2*MTh][KP][PL][64] weight fragments, then cst[Cp/8][6][8] floats
    __shared__ float sm[4];
    __shared__ double red[2][NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.x;
    const int nfrag = 2 * a.MTh * KP * PL * 64;
    for (int i = tid; i < nfrag; i += NW * 64) wl[i] = a.wx[i];
    const int Cp = a.MTh * 32;
    float *cst = reinterpret_cast<float *>(wl + nfrag);  // per-channel constants in LDS: global loads between the gate's stores
    for (int i = tid; i < 6 * Cp; i += NW * 64) cst[i] = a.cst[i];  // could not be hoisted (they may alias), LDS reads can
    SkipNorm nrm;
    slab_mean_inv(a.sy, b, sm, nrm.my, nrm.iy);  // (contains a barrier: the weights are in LDS afterwards)
    const uint4 *xb = a.x + (long)b * a.x_stream;
    const int tiles = (a.TF + 31) >> 5;
    const long plane = a.TF;  // uint4 per plane of one octet

    // B fragments of one position tile: KP K steps x APL planes; lane half h of step kp holds octet 2 kp + h
    // (32-bit offsets from the stream's uniform base here and for ydec and out below: a stream of any of them is below 2^31 bytes)
    auto load_b = [&](int tile, uint4 (&bf)[KP][APL]) {
        const int p = min(tile * 32 + l31, a.TF - 1);
#pragma unroll
        for (int kp = 0; kp < KP; kp++) {
            const int o = min(2 * kp + half, a.C8 - 1);  // a missing odd octet reads a valid one (its weights are zero)
#pragma unroll
            for (int pl = 0; pl < APL; pl++) bf[kp][pl] = xb[(o * APL + pl) * a.TF + p];
        }
    };
    auto mma_tile = [&](int mt, const uint4 (&bf)[KP][APL]) { return skip_mma_tile<PL, KP, FMT, APL>(wl, mt, bf, l31, half); };
    // wl fragment layout per (mt, kp, plane): 64 uint4 = [row 32][k half 2]; lane (row l31, half) reads l31*2 + half

    // ---- pass 1: statistics of residualmask(res) ----
    double s1 = 0, s2 = 0;
    {
        uint4 bcur[KP][APL], bnxt[KP][APL];
        if (wave < tiles) load_b(wave, bcur);
        for (int tile = wave; tile < tiles; tile += NW) {
            if (tile + NW < tiles) load_b(tile + NW, bnxt);
            const bool pos_ok = tile * 32 + l31 < a.TF;
            float ts = 0.0f, tq = 0.0f;
            for (int mt = 0; mt < a.MTh; mt++) skip_stat_tile(cst, mt, half, mma_tile(mt, bcur), ts, tq);
            s1 += pos_ok ? (double)ts : 0.0;  // (a lane beyond the last position computed on a clamped one)
            s2 += pos_ok ? (double)tq : 0.0;
#pragma unroll
            for (int kp = 0; kp < KP; kp++)
#pragma unroll
                for (int pl = 0; pl < APL; pl++) bcur[kp][pl] = bnxt[kp][pl];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (tid == 0) {
        double ts = 0, tq = 0;
        for (int i = 0; i < NW; i++) { ts += red[0][i]; tq += red[1][i]; }
        const double n = (double)a.C * a.TF, m = ts / n;
        double var = tq / n - m * m;
        if (var < 0) var = 0;
        sm[2] = (float)m;
        sm[3] = gln_inv((float)var, a.eps_mode);
    }
    __syncthreads();
    nrm.mu = sm[2]; nrm.iu = sm[3];
    skip_norm_uniform(nrm);
    skip_fold_stats<skip_fast_gate<PL, FMT>()>(cst, Cp, tid, NW * 64, nrm);

    // ---- pass 2: gate ----
    const float invF = 1.0f / (float)a.Fr;
    const float *ydb = a.ydec + (long)b * a.y_stream;
    uint4 *ob = a.out + (long)b * a.out_stream;
    // 16 waves have 128 registers each: there the next tile's fragments are requested into the registers of the current one, once
    // its last MFMA has read them (the gate of the last M tile covers the round trip), and bnxt is not used
    constexpr bool INPLACE = NW == 16;
    uint4 bcur[KP][APL], bnxt[KP][APL];
    if (wave < tiles) load_b(wave, bcur);
    for (int tile = wave; tile < tiles; tile += NW) {
        if (!INPLACE && tile + NW < tiles) load_b(tile + NW, bnxt);
        const int p = tile * 32 + l31;
        const bool pos_ok = p < a.TF;
        const int pc = min(p, a.TF - 1);
        const int t = (int)(((float)pc + 0.5f) * invF), f = pc - t * a.Fr;
        const bool has_y = f < a.Fo;
        const int ypos = t * 2 * a.Fh + (f & 1) * a.Fh + (f >> 1);
        for (int mt = 0; mt < a.MTh; mt++) {
            const f32x16 cm = mma_tile(mt, bcur), cr = mma_tile(a.MTh + mt, bcur);
            if (INPLACE && mt == a.MTh - 1 && tile + NW < tiles) load_b(tile + NW, bcur);
#pragma unroll
            for (int hh = 0; hh < 2; hh++) {
                const int oct = mt * 4 + 2 * half + hh;  // registers 8 hh .. 8 hh + 7 of this lane
                if (oct * 8 >= a.C) continue;
                float yv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (has_y) {
                    const float4 *src = reinterpret_cast<const float4 *>(ydb + (oct * a.T * 2 * a.Fh + ypos) * 8);
                    const float4 u0 = src[0], u1 = src[1];
                    yv[0] = u0.x; yv[1] = u0.y; yv[2] = u0.z; yv[3] = u0.w; yv[4] = u1.x; yv[5] = u1.y; yv[6] = u1.z; yv[7] = u1.w;
                }
                float um[8], ur[8], o[8];
#pragma unroll
                for (int q = 0; q < 8; q++) { um[q] = cm[hh * 8 + q]; ur[q] = cr[hh * 8 + q]; }
                skip_gate_octet<ACT, skip_fast_gate<PL, FMT>()>(cst, oct, a.C - oct * 8, um, ur, yv, has_y, nrm, o);
                if (pos_ok) split_store8_fmt<PL, FMT>(o, ob + (oct * APL * a.TF + p), plane);
            }
        }
        if constexpr (!INPLACE) {
#pragma unroll
            for (int kp = 0; kp < KP; kp++)
#pragma unroll
                for (int pl = 0; pl < APL; pl++) bcur[kp][pl] = bnxt[kp][pl];
        }
    }
}

// ---- the batched form ------------------------------------------------------------------------------------------------------------
// k_skip_p exposes one memory round trip per tile and pass (a wave owns 3 to 6 tiles at the headline shapes, a few dozen MFMAs each:
// the one-ahead prefetch hides nothing), more for the deconvolution values that pass 2 loads where it uses them, and reads res twice.
// k_skip_pd computes the same sums in the same order and changes only WHEN loads are issued:
//     - a wave takes its tiles (wave, wave + NW, ...) in batches of up to DEPTH; all B fragments of a batch are requested before
//       its first MFMA, the first batch before the weight copy and the statistics slab (one round trip for all three)
//     - where every wave's share fits one batch, the fragments stay in registers across the workgroup reduction and
//       pass 2 does not read res again; otherwise pass 2 requests its first batch before the reduction and goes on in batches
//     - pass 2 requests the deconvolution values one tile ahead (the first tile's before the reduction)
// DEPTH: fragment registers of one batch <= 96 of the 256 at 8 waves, <= 24 of the 128 at 16 (12 tiles at the most).
template <int KP, int APL, int NW>
constexpr int skip_depth() {
    const int d = (NW == 8 ? 96 : 24) / (KP * APL * 4);
    return d > 12 ? 12 : (d < 1 ? 1 : d);
}

// `depth` (>= 1) caps a batch below the capacity: SE_SKIP_DEPTH, for tests that want several batches at small shapes.
// MTh follows from KP for every shape the plan admits (KP = 1, 2: C <= 32, one M tile; KP = 4: 49 <= C <= 64, two).
template <int PL, int KP, int NW, int ACT, PlaneFmt FMT = PlaneFmt::kBf16>
__global__ __launch_bounds__(NW * 64) void k_skip_pd(SkipPArgs a, int depth) {
    constexpr bool PAIR = FMT == PlaneFmt::kF16Pair;
    static_assert(!PAIR || PL == kPairPlanesW || PL == kPairPlanesW2, "the fp16 pair form has three weight planes, or two stored ones");
    constexpr int APL = PAIR ? kPairPlanesA : PL;  // planes of res and out
    constexpr int MTH = KP == 4 ? 2 : 1;
    constexpr int DEPTH = skip_depth<KP, APL, NW>();
    constexpr bool UNROLL = DEPTH <= 4;  // the tile loop unrolled where a batch is short: a slot is then used in place, not copied
    extern __shared__ __align__(16) uint4 wl[];  // [2*MTH][KP][PL][64] weight fragments, then cst[Cp/8][6][8] floats
    __shared__ float sm[4];
    __shared__ double red[2][NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.x;
    const uint4 *xb = a.x + (long)b * a.x_stream;
    const int tiles = (a.TF + 31) >> 5;
    const long plane = a.TF;  // uint4 per plane of one octet
    const int nt = wave < tiles ? (tiles - wave + NW - 1) / NW : 0;  // tiles of this wave: wave + k NW, k < nt
    const int dcap = min(depth, DEPTH);
    const bool keep = (tiles + NW - 1) / NW <= dcap;  // (workgroup-uniform: wave 0 owns the most tiles)

    // the B fragments of tiles k0 .. k0 + dcap - 1 of this wave, all requested at once
    uint4 bf[DEPTH][KP][APL];
    auto load_batch = [&](int k0) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            if (d >= dcap || k0 + d >= nt) continue;
            const int p = min((wave + (k0 + d) * NW) * 32 + l31, a.TF - 1);
#pragma unroll
            for (int kp = 0; kp < KP; kp++) {
                const int o = min(2 * kp + half, a.C8 - 1);  // a missing odd octet reads a valid one (its weights are zero)
#pragma unroll
                for (int pl = 0; pl < APL; pl++) bf[d][kp][pl] = xb[((long)o * APL + pl) * plane + p];
            }
        }
    };
    // slot d of the batch (d is wave-uniform; the slots are named at compile time so that they stay registers)
    auto slot = [&](int d, uint4 (&cur)[KP][APL]) {
#pragma unroll
        for (int j = 0; j < DEPTH; j++) {
            if (d != j) continue;
#pragma unroll
            for (int kp = 0; kp < KP; kp++)
#pragma unroll
                for (int pl = 0; pl < APL; pl++) cur[kp][pl] = bf[j][kp][pl];
        }
    };
    auto mma_tile = [&](int mt, const uint4 (&cur)[KP][APL]) { return skip_mma_tile<PL, KP, FMT, APL>(wl, mt, cur, l31, half); };

    // the tiles of one batch in their order: body(slot, k)
    auto for_slots = [&](int k0, auto &&body) {
        if constexpr (UNROLL) {
#pragma unroll
            for (int d = 0; d < DEPTH; d++)
                if (d < dcap && k0 + d < nt) body(d, k0 + d);
        } else {
#pragma nounroll
            for (int d = 0; d < dcap && k0 + d < nt; d++) body(d, k0 + d);
        }
    };

    load_batch(0);
    const int nfrag = 2 * MTH * KP * PL * 64;
    for (int i = tid; i < nfrag; i += NW * 64) wl[i] = a.wx[i];
    constexpr int Cp = MTH * 32;
    float *cst = reinterpret_cast<float *>(wl + nfrag);
    for (int i = tid; i < 6 * Cp; i += NW * 64) cst[i] = a.cst[i];
    SkipNorm nrm;
    slab_mean_inv(a.sy, b, sm, nrm.my, nrm.iy);  // (contains a barrier: the weights are in LDS afterwards)

    // ---- pass 1: statistics of residualmask(res); float per tile, double across a wave's tiles in their order ----
    double s1 = 0, s2 = 0;
    auto stat_tile = [&](int d, int k) {
        uint4 cur[KP][APL];
        slot(d, cur);
        const bool pos_ok = (wave + k * NW) * 32 + l31 < a.TF;
        float ts = 0.0f, tq = 0.0f;
#pragma nounroll
        for (int mt = 0; mt < MTH; mt++) {  // (not unrolled: the code of an unrolled batch stays within the instruction cache)
            skip_stat_tile(cst, mt, half, mma_tile(mt, cur), ts, tq);
        }
        s1 += pos_ok ? (double)ts : 0.0;  // (a lane beyond the last position computed on a clamped one)
        s2 += pos_ok ? (double)tq : 0.0;
    };
    for (int k0 = 0; k0 < nt; k0 += dcap) {
        if (k0) load_batch(k0);
        for_slots(k0, stat_tile);
    }
    if (!keep) load_batch(0);  // pass 2's first batch: in flight across the reduction

    // A lane gates NH octets of 8 channels per M tile: registers 8 hh .. 8 hh + 7 are octet mt * 4 + 2 half + hh.  KP = 1 (C <= 16) has
    // octets 0 and 1 only, both in lane half 0, and the whole wave would issue the gate of 16 values for half its lanes: there lane
    // half 1 takes octet 1 over from its partner lane (the same position), and every lane gates one octet.
    constexpr bool SPLIT = KP == 1;
    constexpr int NH = SPLIT ? 1 : 2;
    // the deconvolution values of one M tile of one position tile: [hh] octets of 8 channels, fp32
    const float invF = 1.0f / (float)a.Fr;
    const float *ydb = a.ydec + (long)b * a.y_stream;
    auto load_y = [&](int k, int mt, float4 (&y)[2][2]) {
        const int pc = min((wave + k * NW) * 32 + l31, a.TF - 1);
        const int t = (int)(((float)pc + 0.5f) * invF), f = pc - t * a.Fr;
        const long ypos = (long)t * 2 * a.Fh + (f & 1) * a.Fh + (f >> 1);
#pragma unroll
        for (int hh = 0; hh < NH; hh++) {
            const int oct = SPLIT ? half : mt * 4 + 2 * half + hh;
            y[hh][0] = y[hh][1] = make_float4(0, 0, 0, 0);
            if (f < a.Fo && oct * 8 < a.C) {
                const float4 *src = reinterpret_cast<const float4 *>(ydb + ((long)oct * a.T * 2 * a.Fh + ypos) * 8);
                y[hh][0] = src[0];
                y[hh][1] = src[1];
            }
        }
    };
    float4 ycur[2][2], ynxt[2][2];
    if (nt > 0) load_y(0, 0, ycur);  // (they do not depend on the mask statistics)

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (tid == 0) {
        double ts = 0, tq = 0;
        for (int i = 0; i < NW; i++) { ts += red[0][i]; tq += red[1][i]; }
        const double n = (double)a.C * a.TF, m = ts / n;
        double var = tq / n - m * m;
        if (var < 0) var = 0;
        sm[2] = (float)m;
        sm[3] = gln_inv((float)var, a.eps_mode);
    }
    __syncthreads();
    nrm.mu = sm[2]; nrm.iu = sm[3];
    skip_norm_uniform(nrm);
    skip_fold_stats<skip_fast_gate<PL, FMT>()>(cst, Cp, tid, NW * 64, nrm);

    // ---- pass 2: gate ----
    uint4 *ob = a.out + (long)b * a.out_stream;
    auto gate_tile = [&](int d, int k) {
        uint4 cur[KP][APL];
        slot(d, cur);
        const int p = (wave + k * NW) * 32 + l31;
        const bool pos_ok = p < a.TF;
        const int pc = min(p, a.TF - 1);
        const int t = (int)(((float)pc + 0.5f) * invF), f = pc - t * a.Fr;
        const bool has_y = f < a.Fo;
#pragma nounroll
        for (int mt = 0; mt < MTH; mt++) {  // (not unrolled: the code of an unrolled batch stays within the instruction cache)
            if (mt + 1 < MTH) load_y(k, mt + 1, ynxt);  // one step ahead: the tile's next M tile, or the next tile's first
            else if (k + 1 < nt) load_y(k + 1, 0, ynxt);
            const f32x16 cm = mma_tile(mt, cur), cr = mma_tile(MTH + mt, cur);
#pragma unroll
            for (int hh = 0; hh < NH; hh++) {
                const int oct = SPLIT ? half : mt * 4 + 2 * half + hh;
                float um[8], ur[8];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    um[q] = cm[hh * 8 + q];
                    ur[q] = cr[hh * 8 + q];
                    if constexpr (SPLIT) {  // (every lane of the wave is here: the exchange sits outside the octet test)
                        const float tm = __shfl_xor(cm[8 + q], 32, 64), tr = __shfl_xor(cr[8 + q], 32, 64);
                        if (half) { um[q] = tm; ur[q] = tr; }
                    }
                }
                if (oct * 8 >= a.C) continue;
                const float4 u0 = ycur[hh][0], u1 = ycur[hh][1];
                const float yv[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
                float o[8];
                skip_gate_octet<ACT, skip_fast_gate<PL, FMT>()>(cst, oct, a.C - oct * 8, um, ur, yv, has_y, nrm, o);
                if (pos_ok) split_store8_fmt<PL, FMT>(o, ob + (long)oct * APL * plane + p, plane);
            }
#pragma unroll
            for (int hh = 0; hh < NH; hh++) { ycur[hh][0] = ynxt[hh][0]; ycur[hh][1] = ynxt[hh][1]; }
        }
    };
    for (int k0 = 0; k0 < nt; k0 += dcap) {
        if (k0) load_batch(k0);
        for_slots(k0, gate_tile);
    }
}

}  // namespace se
