// pair_w2_check.cpp - host check of the fp16 pair's two STORED weight planes (csrc/split_f16pair.h: pair_weight_planes2 and
// pair_scale_hi_bits; csrc/gru_pack.h: gru_pack_whh_pair2; csrc/conv_weight_image.h with PL = 2).
// Plain C++: g++ -O2 -std=c++17 pair_w2_check.cpp && ./a.out.  Exit status 0 = every check held.
//
// 1. For every fp16 bit pattern h with |h| < 2^4 (zeros and every subnormal included): what the kernels compute from a stored w_hi = h,
//    ONE fp16 multiply by 2^11, equals plane 0 of pair_weight_planes for a weight whose high part is h.  The multiply is done here
//    on the compiler's _Float16 where it has one (the arithmetic of v_pk_mul_f16: round to nearest even, subnormals kept) and through
//    pair_scale_hi_bits; both must agree.
// 2. The two-plane conv, skip, matrix and W_hh images equal planes 1 and 2 of the three-plane images at the indices the kernels read.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../speech_enhancement_mi_amd/csrc/conv_weight_image.h"
#include "../speech_enhancement_mi_amd/csrc/gru_pack.h"
#include "../speech_enhancement_mi_amd/csrc/split_f16pair.h"

using namespace se;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            g_fail++;                                     \
        }                                                 \
    } while (0)

static uint64_t g_seed = 0x2545f4914f6cdd1dull;
static double uniform() {  // [0, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}

// weights like the GPU test's edited checkpoint: ordinary values, a tenth with an fp16-subnormal high part, a tenth exact +-0, a few +-15.9
static float weight() {
    const double u = uniform();
    const float sign = uniform() < 0.5 ? -1.0f : 1.0f;
    if (u < 0.1) return sign * (float)std::exp(std::log(1e-7) + uniform() * (std::log(1e-4) - std::log(1e-7)));
    if (u < 0.2) return sign * 0.0f;
    if (u < 0.22) return sign * 15.9f;
    return sign * (float)(uniform() * 0.5);
}

static uint16_t device_scale(uint16_t hi) {
#if defined(__FLT16_MANT_DIG__)
    _Float16 h;
    memcpy(&h, &hi, 2);
    const _Float16 p = h * (_Float16)2048.0f;  // one fp16 multiply
    uint16_t r;
    memcpy(&r, &p, 2);
    return r;
#else
    return pair_scale_hi_bits(hi);
#endif
}

int main() {
    // ---- 1. the device scale on every fp16 below 2^4, both signs
    int n_sub = 0, n_all = 0;
    for (uint32_t h = 0; h < 0x10000u; h++) {
        const uint16_t hb = (uint16_t)h;
        const float v = pair_f16_value(hb);
        if (!(std::fabs(v) < 16.0f)) continue;  // (drops inf / NaN too)
        n_all++;
        n_sub += ((hb >> 10) & 31) == 0;
        // a weight whose high part is h: v itself (fp16(v) == v).  No weight has the high part -0 (split2h stores zero as +0, +0): for
        // that one pattern the multiply is checked against plane 0's own expression, fp16(value(h) * 2^11) = -0
        uint16_t hi, lo;
        split2h(v, hi, lo);
        if (hb == 0x8000u) {
            CHECK(hi == 0 && lo == 0, "split2h(-0) = (%04x, %04x)", hi, lo);
            CHECK(device_scale(hb) == 0x8000u && pair_scale_hi_bits(hb) == 0x8000u, "-0 * 2^11 gives %04x / %04x", device_scale(hb), pair_scale_hi_bits(hb));
            continue;
        }
        CHECK(hi == hb, "split2h(%.9g) has hi %04x, expected %04x", v, hi, hb);
        uint16_t p[3], q[2];
        pair_weight_planes(v, p);
        pair_weight_planes2(v, q);
        CHECK(q[0] == p[1] && q[1] == p[2], "two planes of %.9g: (%04x %04x), three: (%04x %04x %04x)", v, q[0], q[1], p[0], p[1], p[2]);
        CHECK(device_scale(q[1]) == p[0], "fp16 multiply of %04x by 2^11 gives %04x, plane 0 is %04x", q[1], device_scale(q[1]), p[0]);
        CHECK(pair_scale_hi_bits(q[1]) == p[0], "pair_scale_hi_bits(%04x) = %04x, plane 0 is %04x", q[1], pair_scale_hi_bits(q[1]), p[0]);
        CHECK(((p[0] >> 10) & 31) != 31, "plane 0 of %.9g is not finite", v);
    }
    CHECK(n_sub == 2048 && n_all == 2 * (19 << 10), "covered %d patterns, %d subnormal or zero", n_all, n_sub);
    // random weights with a low part as well: the stored high part scales to plane 0
    for (int i = 0; i < 200000; i++) {
        const float w = weight();
        uint16_t p[3], q[2];
        pair_weight_planes(w, p);
        pair_weight_planes2(w, q);
        CHECK(q[0] == p[1] && q[1] == p[2] && device_scale(q[1]) == p[0], "weight %.9g", w);
    }

    // ---- 2a. matrix planes [2][n] against planes 1, 2 of [3][n]
    {
        const size_t n = 24 * 40;
        std::vector<float> w(n);
        for (auto &x : w) x = weight();
        std::vector<uint16_t> p3(3 * n), p2(2 * n);
        pair_weight_matrix(w.data(), n, p3.data());
        pair_weight_matrix2(w.data(), n, p2.data());
        for (size_t i = 0; i < n; i++)
            CHECK(p2[i] == p3[n + i] && p2[n + i] == p3[2 * n + i], "matrix element %zu", i);
    }
    // ---- 2b. packed W_hh: six fragments per k step against slots 1, 2 of the nine
    {
        const int H = 64;
        std::vector<float> w((size_t)3 * H * H);
        for (auto &x : w) x = weight();
        std::vector<uint16_t> k3, k2;
        gru_pack_whh_pair(w.data(), H, k3);
        gru_pack_whh_pair2(w.data(), H, k2);
        CHECK(k3.size() == gru_pack_size(H) && k2.size() == gru_pack_size(H, 2) && 3 * k2.size() == 2 * k3.size(), "packed sizes %zu, %zu", k3.size(), k2.size());
        std::vector<char> seen(k2.size(), 0);
        for (int g = 0; g < 3; g++)
            for (int n = 0; n < H; n++)
                for (int k = 0; k < H; k++)
                    for (int pl = 0; pl < 2; pl++) {
                        const size_t i2 = gru_pack_index(H, g, n, k, pl, 2), i3 = gru_pack_index(H, g, n, k, pl + 1);
                        CHECK(i2 < k2.size() && !seen[i2], "W_hh index (%d, %d, %d, %d) out of range or used twice", g, n, k, pl);
                        if (i2 >= k2.size()) continue;
                        seen[i2] = 1;
                        CHECK(k2[i2] == k3[i3], "W_hh (%d, %d, %d) plane %d", g, n, k, pl);
                    }
        // the fragment order the kernel walks: [unit group][k step][gate][plane][lane][8]
        CHECK(gru_pack_index(H, 1, 33, 17, 1, 2) == ((((size_t)1 * (H / 16) + 1) * 3 + 1) * 2 + 1) * 512 + (size_t)(0 * 32 + 1) * 8 + 1, "fragment order");
    }
    // ---- 2c. conv image (9 taps, 24 -> 40 channels: two M tiles, three chunks) and 2d. skip image (40 channels: KP = 3 steps, odd octet)
    {
        const int Ci = 24, Co = 40, CoPad = 64, CO = 1, nchunk = 3, ntap = 9, npair = (ntap * CO + 1) / 2, MT = CoPad / 32;
        std::vector<float> w((size_t)Co * Ci * ntap);
        for (auto &x : w) x = weight();
        std::vector<std::array<int, 4>> taps;
        for (int t = 0; t < ntap; t++) taps.push_back({t / 3, t % 3, 0, 0});
        auto wsel = [&](int ci, int row, int kf, int kt) { return w[((size_t)row * Ci + ci) * ntap + kf * 3 + kt]; };
        for (int mode : {(int)kPOutR, (int)kPOutP, (int)kPOutBlend}) {
            const auto i3 = convp_weight_image(mode, CO, nchunk, Ci, Co, CoPad, 3, taps, wsel, [](float x, uint16_t (&p)[3]) { pair_weight_parts(x, 3, p); });
            const auto i2 = convp_weight_image(mode, CO, nchunk, Ci, Co, CoPad, 2, taps, wsel, [](float x, uint16_t (&p)[3]) { pair_weight_parts(x, 2, p); });
            CHECK(3 * i2.size() == 2 * i3.size(), "conv image sizes %zu, %zu", i2.size(), i3.size());
            int nonzero = 0;
            for (int ch = 0; ch < nchunk; ch++)
                for (int pr = 0; pr < npair; pr++)
                    for (int m = 0; m < MT; m++)
                        for (int r = 0; r < 32; r++)
                            for (int k = 0; k < 16; k++)
                                for (int pl = 0; pl < 2; pl++) {
                                    const uint16_t a = i2[convp_weight_index(npair, 2, MT, ch, pr, pl, m, r, k)], b = i3[convp_weight_index(npair, 3, MT, ch, pr, pl + 1, m, r, k)];
                                    CHECK(a == b, "conv image mode %d (%d, %d, %d, %d, %d) plane %d", mode, ch, pr, m, r, k, pl);
                                    nonzero += a != 0;
                                    if (pl == 1) CHECK(device_scale(a) == i3[convp_weight_index(npair, 3, MT, ch, pr, 0, m, r, k)], "conv image plane 0");
                                }
            CHECK(nonzero > 1000, "conv image mode %d is empty", mode);
        }
        const int C = 40, MTh = 2, KP = 3;
        std::vector<float> mw((size_t)C * C), rw((size_t)C * C);
        for (auto &x : mw) x = weight();
        for (auto &x : rw) x = weight();
        const auto s3 = skip_weight_image(C, MTh, KP, 3, mw.data(), rw.data(), [](float x, uint16_t (&p)[3]) { pair_weight_parts(x, 3, p); });
        const auto s2 = skip_weight_image(C, MTh, KP, 2, mw.data(), rw.data(), [](float x, uint16_t (&p)[3]) { pair_weight_parts(x, 2, p); });
        CHECK(3 * s2.size() == 2 * s3.size(), "skip image sizes %zu, %zu", s2.size(), s3.size());
        for (int m2 = 0; m2 < 2 * MTh; m2++)
            for (int kp = 0; kp < KP; kp++)
                for (int r = 0; r < 32; r++)
                    for (int k = 0; k < 16; k++)
                        for (int pl = 0; pl < 2; pl++)
                            CHECK(s2[skip_weight_index(KP, 2, m2, kp, pl, r, k)] == s3[skip_weight_index(KP, 3, m2, kp, pl + 1, r, k)], "skip image (%d, %d, %d, %d) plane %d", m2, kp, r, k, pl);
    }
    printf("%s: %d fp16 patterns below 2^4 (%d zero or subnormal), images checked, %d failures\n", g_fail ? "FAILED" : "ok", n_all, n_sub, g_fail);
    return g_fail ? 1 : 0;
}
