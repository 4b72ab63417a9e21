// conv_weight_image.h - host side of the plane-layout convolution path that needs no HIP: the weight fragment images k_conv_p and
// k_skip_p read, at the indices they read them, and the range bound of a skip output for the fp16 pair format (split_f16pair.h).
// Plain C++: convp_engine.inc.h / se_engine.hip and tests/f16_pair_conv_check.cpp compile the same code.
//
// The images are the same in every operand format; what a format decides is the contents of the planes of one weight, which the
// caller passes as `parts(w, p[3])`: (hi, mid, lo) bf16 for the split-bf16 route, one fp16 number, or pair_weight_planes'
// (2^11 w_hi, w_lo, w_hi).
#pragma once
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "split_f16pair.h"

namespace se {

enum ConvPOut : int { kPOutR = 0, kPOutP = 1, kPOutBlend = 2, kPOutStats = 3, kPOutGate = 4, kPOutPre = 5 };

// GEMM row -> logical row of the caller's weight selector, for the epilogue's register ownership (conv_p.hip.h)
inline int convp_row_logical(int mode, int row) {
    const int mt = row >> 5, rp = row & 31, h = (rp >> 2) & 1, r = (rp & 3) + 4 * (rp >> 3);
    if (mode == kPOutPre) return (mt == 0 && h == 0 && r < 8) ? r : (1 << 20);  // channels 0-7 = registers 0-7 of lane half 0
    if (mode == kPOutP) return mt * 32 + 16 * h + r;                       // registers 0..15 of half h = channels 16 h + r
    if (mode == kPOutBlend || mode == kPOutGate) return 2 * (mt * 16 + 8 * h + (r >> 1)) + (r & 1);  // pairs (residualmask, residual) / (trans, gated) of channel 8 h + r/2
    return row;
}

// k_conv_p: [chunk][pair][plane][mtile][row 32][k 16], k = half*8 + c <-> entry 2*pair + half = (tap, octet) tap-major
inline size_t convp_weight_index(int npair, int PL, int MT, int ch, int pr, int plane, int m, int r, int k) {
    return (((((size_t)ch * npair + pr) * PL + plane) * MT + m) * 32 + r) * 16 + k;
}

// taps[t] = (kf, kt, row group, column offset); wsel(ci, logical row, kf, kt) fetches the reference weight
template <class WSel, class Parts>
std::vector<uint16_t> convp_weight_image(int out_mode, int CO, int nchunk, int Ci, int Co, int CoPad, int PL,
                                         const std::vector<std::array<int, 4>> &taps, WSel wsel, Parts parts) {
    const int ntap = (int)taps.size(), npair = (ntap * CO + 1) / 2, MT = CoPad / 32;
    std::vector<uint16_t> wx((size_t)nchunk * npair * PL * MT * 32 * 16, 0);
    for (int ch = 0; ch < nchunk; ch++)
        for (int st = 0; st < npair; st++)
            for (int m = 0; m < MT; m++)
                for (int r = 0; r < 32; r++) {
                    const int lg = convp_row_logical(out_mode, m * 32 + r);
                    if (lg >= Co) continue;
                    for (int k = 0; k < 16; k++) {
                        const int en = 2 * st + k / 8, tp = en / CO, oc = en % CO;
                        const int ci = (ch * CO + oc) * 8 + k % 8;
                        if (tp >= ntap || ci >= Ci) continue;
                        uint16_t p[3];
                        parts(wsel(ci, lg, taps[tp][0], taps[tp][1]), p);
                        for (int pln = 0; pln < PL; pln++) wx[convp_weight_index(npair, PL, MT, ch, st, pln, m, r, k)] = p[pln];
                    }
                }
    return wx;
}

// k_skip_p: [m2][kp][plane][row 32][k 16]; M tiles [0, MTh) = residualmask rows, [MTh, 2 MTh) = residual rows, rows permuted like
// kPOutP; lane half h of K step kp holds octet 2 kp + h
inline size_t skip_weight_index(int KP, int PL, int m2, int kp, int plane, int r, int k) {
    return ((((size_t)m2 * KP + kp) * PL + plane) * 32 + r) * 16 + k;
}

template <class Parts>
std::vector<uint16_t> skip_weight_image(int Co, int MTh, int KP, int PL, const float *maskw, const float *resw, Parts parts) {
    std::vector<uint16_t> wx((size_t)2 * MTh * KP * PL * 32 * 16, 0);
    for (int m2 = 0; m2 < 2 * MTh; m2++)
        for (int kp = 0; kp < KP; kp++)
            for (int r = 0; r < 32; r++) {
                const int mt = m2 % MTh, kind = m2 / MTh;
                const int ch = convp_row_logical(kPOutP, mt * 32 + r);
                if (ch >= Co) continue;
                for (int k = 0; k < 16; k++) {
                    const int ci = (2 * kp + k / 8) * 8 + k % 8;
                    if (ci >= Co) continue;
                    uint16_t p[3];
                    parts(kind ? resw[(size_t)ch * Co + ci] : maskw[(size_t)ch * Co + ci], p);
                    for (int pln = 0; pln < PL; pln++) wx[skip_weight_index(KP, PL, m2, kp, pln, r, k)] = p[pln];
                }
            }
    return wx;
}

// ---- range bounds of the fp16 pair format (decided once per weight load: se_engine.hip, f16_pair_guard) ----
constexpr double kPairGuardLimit = 6.0e4;

// what a global layer norm over n elements per stream can write: |x - mean| <= sqrt(n) sigma
inline double pair_norm_bound(double gamma_max, double beta_max, double n) { return gamma_max * std::sqrt(n) + beta_max; }

// The skip output of a decoder level, out = g act(residual(res)) + (1 - g) pad(norm(act(deconv))) with g in (0, 1), is a convex
// combination of its two branches (|act(v)| <= |v| for ReLU and ELU): its bound is the larger of the decoder norm's bound and, for
// the 1x1 branch, (largest row L1 norm of residual.weight [C][C]) x (bound of res, the encoder norm's) + max|bias|.  NaN / inf
// parameters give an infinite bound.
inline double pair_skip_bound(const float *resw, const float *resb, int C, double res_bound, double dec_norm_bound) {
    double l1max = 0, bmax = 0;
    for (int r = 0; r < C; r++) {
        double l1 = 0;
        for (int c = 0; c < C; c++) l1 += std::fabs((double)resw[(size_t)r * C + c]);
        if (!(l1 <= 1e300)) return INFINITY;
        l1max = l1 > l1max ? l1 : l1max;
        const double b = std::fabs((double)resb[r]);
        if (!(b <= 1e300)) return INFINITY;
        bmax = b > bmax ? b : bmax;
    }
    const double branch = l1max * res_bound + bmax;
    return branch > dec_norm_bound ? branch : dec_norm_bound;
}

}  // namespace se
