// gru_pack.h - host packing of W_hh for the split-bf16 GRU step (gemm.hip.h: gru_split_body).  Plain C++, no HIP: the same code
// runs in the engine's weight preparation and in tests/gru_pack_check.cpp.
//
// W_hh [3H][H] fp32 (gate order r, z, n) becomes three bf16 planes (hi, mid, lo; hi + mid + lo == w exactly, as split3 does on the
// device) stored in the order the kernel's waves consume them.  A fragment is the B operand of one v_mfma_f32_32x32x16_bf16: 32
// hidden units x 16 k, lane (k half h, unit r) = 32 h + r holding the 8 bf16 of k = 8 h .. 8 h + 7 - 64 lanes x 16 bytes, contiguous:
//   [unit group n / 32][k step k / 16][gate][plane][lane 32 ((k / 8) & 1) + n % 32][k % 8]
// so a wave's nine fragments of a k step are one 9-KB run and every fragment load is one 1-KB read.  Requires H % 32 == 0.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "split_f16pair.h"

namespace se {

inline uint16_t gru_pack_bf16_rne(float x) {  // round to nearest even, as engine_host.h: bf16_rne
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float gru_pack_bf16_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// position (in bf16 elements) of plane `pl` of W_hh[gate * H + n][k] in the packed image; NP = stored planes per gate (three, or the
// two of gru_pack_whh_pair2: six fragments per k step)
inline size_t gru_pack_index(int H, int gate, int n, int k, int pl, int NP = 3) {
    const size_t frag = (((size_t)(n >> 5) * (H >> 4) + (k >> 4)) * 3 + gate) * NP + pl;
    const int lane = 32 * ((k >> 3) & 1) + (n & 31);
    return (frag * 64 + lane) * 8 + (k & 7);
}

inline size_t gru_pack_size(int H, int NP = 3) { return (size_t)3 * NP * H * H; }  // bf16 elements

inline void gru_pack_whh(const float *whh, int H, std::vector<uint16_t> &out) {
    out.assign(gru_pack_size(H), 0);
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++) {
                const float x = whh[((size_t)g * H + n) * H + k];
                const uint16_t h = gru_pack_bf16_rne(x);
                const float r1 = x - gru_pack_bf16_f32(h);
                const uint16_t m = gru_pack_bf16_rne(r1);
                const uint16_t l = gru_pack_bf16_rne(r1 - gru_pack_bf16_f32(m));
                out[gru_pack_index(H, g, n, k, 0)] = h;
                out[gru_pack_index(H, g, n, k, 1)] = m;
                out[gru_pack_index(H, g, n, k, 2)] = l;
            }
}

// the same image for the fp16 pair format (split_f16pair.h): plane slots 0, 1, 2 of every fragment hold (2^11 hi, lo, hi) as fp16
inline void gru_pack_whh_pair(const float *whh, int H, std::vector<uint16_t> &out) {
    out.assign(gru_pack_size(H), 0);
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++) {
                uint16_t p[3];
                pair_weight_planes(whh[((size_t)g * H + n) * H + k], p);
                for (int pl = 0; pl < 3; pl++) out[gru_pack_index(H, g, n, k, pl)] = p[pl];
            }
}

// the pair image with the two STORED planes (split_f16pair.h: pair_weight_planes2): slots 0, 1 of every gate hold (lo, hi)
inline void gru_pack_whh_pair2(const float *whh, int H, std::vector<uint16_t> &out) {
    out.assign(gru_pack_size(H, kPairPlanesW2), 0);
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++) {
                uint16_t p[2];
                pair_weight_planes2(whh[((size_t)g * H + n) * H + k], p);
                for (int pl = 0; pl < 2; pl++) out[gru_pack_index(H, g, n, k, pl, kPairPlanesW2)] = p[pl];
            }
}

}  // namespace se
