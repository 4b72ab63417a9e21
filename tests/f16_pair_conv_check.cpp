// f16_pair_conv_check.cpp - host check of the fp16 pair format on the convolution / skip path (csrc/conv_weight_image.h,
// csrc/split_f16pair.h): the k_conv_p and k_skip_p weight images at the indices the kernels read, the skip output's range bound, and
// split2h(join2h(.)) as the identity on stored pairs.  Plain C++: g++ -O2 -std=c++17 f16_pair_conv_check.cpp && ./a.out.
// Exit status 0 = every check held.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../speech_enhancement_mi_amd/csrc/conv_weight_image.h"
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
static float weight() {  // log-uniform magnitude up to just under 2^4 (the guard's limit), both signs
    const double mag = std::exp2(-20.0 + uniform() * 23.9);
    return (float)(uniform() < 0.5 ? -mag : mag);
}

static void pair_parts(float x, uint16_t (&p)[3]) { pair_weight_planes(x, p); }

// One k_conv_p geometry: the image holds (2^11 w_hi, w_lo, w_hi) of weight (ci, logical row, tap) at
// (((ch NPAIR + pr) 3 + plane) MT + m) 64 uint4 + the lane's piece, i.e. uint16 index ((... MT + m) 32 + r) 16 + k, and zero elsewhere
static void check_conv(const char *what, int out_mode, int ntap, int Ci, int Co) {
    const int C8 = (Ci + 7) / 8;
    int CO = 1;
    if (ntap == 1) CO = C8 >= 4 ? 4 : (C8 >= 2 ? 2 : 1);
    while (C8 % CO) CO /= 2;
    const int nchunk = C8 / CO, npair = (ntap * CO + 1) / 2, CoPad = (Co + 31) / 32 * 32, MT = CoPad / 32;
    std::vector<std::array<int, 4>> taps;
    for (int t = 0; t < ntap; t++) taps.push_back({t / 3, t % 3, t % 3, t / 3});
    std::vector<float> w((size_t)Co * Ci * ntap);
    for (float &x : w) x = weight();
    w[0] = 15.999f;
    auto wsel = [&](int ci, int row, int kf, int kt) { return w[((size_t)row * Ci + ci) * ntap + kf * 3 + kt]; };
    const std::vector<uint16_t> img = convp_weight_image(out_mode, CO, nchunk, Ci, Co, CoPad, 3, taps, wsel, pair_parts);
    CHECK(img.size() == (size_t)nchunk * npair * 3 * MT * 64 * 8, "%s: image size", what);
    size_t nonzero_expected = 0, checked = 0;
    for (int ch = 0; ch < nchunk; ch++)
        for (int pr = 0; pr < npair; pr++)
            for (int m = 0; m < MT; m++)
                for (int r = 0; r < 32; r++)
                    for (int k = 0; k < 16; k++) {
                        // what the kernel's lane (l31 = r, half = k / 8) multiplies: entry 2 pr + half = (tap, octet) tap-major, channel k % 8
                        const int en = 2 * pr + k / 8, tp = en / CO, oc = en % CO, ci = (ch * CO + oc) * 8 + k % 8;
                        const int lg = convp_row_logical(out_mode, m * 32 + r);
                        const bool live = lg < Co && tp < ntap && ci < Ci;
                        uint16_t want[3] = {0, 0, 0}, hi = 0, lo = 0;
                        if (live) {
                            const float x = wsel(ci, lg, taps[tp][0], taps[tp][1]);
                            split2h(x, hi, lo);
                            want[0] = pair_f16_bits(2048.0f * pair_f16_value(hi)); want[1] = lo; want[2] = hi;
                            CHECK(((want[0] >> 10) & 31) != 31, "%s: 2^11 w_hi of %g overflows", what, x);
                            nonzero_expected++;
                        }
                        for (int pl = 0; pl < 3; pl++) {
                            const size_t idx = (((((size_t)ch * npair + pr) * 3 + pl) * MT + m) * 64 + (size_t)r * 2 + k / 8) * 8 + k % 8;  // uint4 piece, then channel
                            CHECK(idx == convp_weight_index(npair, 3, MT, ch, pr, pl, m, r, k), "%s: index form", what);
                            CHECK(img[idx] == want[pl], "%s: chunk %d pair %d plane %d tile %d row %d k %d: %04x, expected %04x", what, ch, pr, pl, m, r, k, img[idx], want[pl]);
                            checked++;
                        }
                    }
    CHECK(checked == img.size(), "%s: every element visited", what);
    CHECK(nonzero_expected == (size_t)Co * Ci * ntap, "%s: every weight placed exactly once (%zu of %zu)", what, nonzero_expected, (size_t)Co * Ci * ntap);
}

static void check_skip(int Co) {
    const int C8 = (Co + 7) / 8, MTh = (Co + 31) / 32, KP = (C8 + 1) / 2;
    std::vector<float> mw((size_t)Co * Co), rw((size_t)Co * Co);
    for (float &x : mw) x = weight();
    for (float &x : rw) x = weight();
    const std::vector<uint16_t> img = skip_weight_image(Co, MTh, KP, 3, mw.data(), rw.data(), pair_parts);
    CHECK(img.size() == (size_t)2 * MTh * KP * 3 * 64 * 8, "skip %d: image size", Co);
    size_t placed = 0;
    for (int m2 = 0; m2 < 2 * MTh; m2++)
        for (int kp = 0; kp < KP; kp++)
            for (int r = 0; r < 32; r++)
                for (int k = 0; k < 16; k++) {
                    // k_skip_p: wl + ((mt KP + kp) PL + plane) 64 + l31 2 + half; lane half h of step kp holds octet 2 kp + h; register r of lane
                    // half h is channel mt 32 + 16 h + r (the kPOutP permutation)
                    const int mt = m2 % MTh, kind = m2 / MTh, ch = convp_row_logical(kPOutP, mt * 32 + r), ci = (2 * kp + k / 8) * 8 + k % 8;
                    const bool live = ch < Co && ci < Co;
                    uint16_t want[3] = {0, 0, 0};
                    if (live) {
                        uint16_t hi, lo;
                        split2h(kind ? rw[(size_t)ch * Co + ci] : mw[(size_t)ch * Co + ci], hi, lo);
                        want[0] = pair_f16_bits(2048.0f * pair_f16_value(hi)); want[1] = lo; want[2] = hi;
                        placed++;
                    }
                    for (int pl = 0; pl < 3; pl++) {
                        const size_t idx = ((((size_t)m2 * KP + kp) * 3 + pl) * 64 + (size_t)r * 2 + k / 8) * 8 + k % 8;
                        CHECK(idx == skip_weight_index(KP, 3, m2, kp, pl, r, k), "skip %d: index form", Co);
                        CHECK(img[idx] == want[pl], "skip %d: tile %d step %d plane %d row %d k %d", Co, m2, kp, pl, r, k);
                    }
                }
    CHECK(placed == (size_t)2 * Co * Co, "skip %d: every weight placed exactly once", Co);
}

int main() {
    // ---- weight images: one geometry per tap count 15, 9, 6 and 1, an odd octet count, the permuted epilogues
    check_conv("15 taps, 16 -> 32, R", kPOutR, 15, 16, 32);
    check_conv("9 taps, 64 -> 32, R", kPOutR, 9, 64, 32);
    check_conv("6 taps, 24 -> 16 (3 octets), R", kPOutR, 6, 24, 16);
    check_conv("15 taps, 20 -> 4 (partial octet)", kPOutR, 15, 20, 4);
    check_conv("1 tap, 32 -> 64, blend", kPOutBlend, 1, 32, 64);
    check_conv("1 tap, 24 -> 48 (3 octets), blend", kPOutBlend, 1, 24, 48);
    check_conv("1 tap, 16 -> 16, P", kPOutP, 1, 16, 16);
    check_skip(64);
    check_skip(32);
    check_skip(16);
    check_skip(8);
    check_skip(24);  // 3 octets: the odd half of the last K step is padding

    // ---- the skip output's bound (pair_skip_bound): the larger of the decoder norm's bound and row L1 norm x bound of res + max|bias|
    {
        const int C = 64;
        std::vector<float> w((size_t)C * C, 0.01f), b(C, 0.0f);
        const double res_bound = pair_norm_bound(1.2, 0.1, 64.0 * 21 * 17), dec_bound = pair_norm_bound(1.0, 0.2, 64.0 * 21 * 33);
        CHECK(std::fabs(res_bound - (1.2 * std::sqrt(64.0 * 21 * 17) + 0.1)) < 1e-9, "norm bound");
        // small weights: the decoder norm's branch is the larger one
        CHECK(pair_skip_bound(w.data(), b.data(), C, res_bound, dec_bound) == dec_bound, "small 1x1 weights: the norm branch bounds the output");
        // one row of 15.0: every weight is below 16, no norm changed, and the row's L1 norm 960 times the bound of res crosses 6e4
        for (int c = 0; c < C; c++) w[(size_t)7 * C + c] = 15.0f;
        const double crossed = pair_skip_bound(w.data(), b.data(), C, res_bound, dec_bound);
        CHECK(std::fabs(crossed - 960.0 * res_bound) < 1e-6 * crossed && crossed > kPairGuardLimit, "row of 15.0: bound %g", crossed);
        // just below the limit: scale that row so that L1 x res_bound + |bias| = 0.999 x 6e4
        b[7] = -3.0f;
        const float each = (float)((0.999 * kPairGuardLimit - 3.0) / res_bound / C);
        for (int c = 0; c < C; c++) w[(size_t)7 * C + c] = (c & 1) ? -each : each;  // signs do not matter to an L1 norm
        const double below = pair_skip_bound(w.data(), b.data(), C, res_bound, dec_bound);
        CHECK(below <= kPairGuardLimit && below > 0.998 * kPairGuardLimit, "just below the limit: bound %g", below);
        w[5] = NAN;
        CHECK(!(pair_skip_bound(w.data(), b.data(), C, res_bound, dec_bound) <= kPairGuardLimit), "a NaN weight fails the bound");
    }

    // ---- split2h(join2h(.)) is the identity on stored pairs: what export_state / import_state of a conv history rely on.  The pairs
    // just below a tie of the fp16 grid (low part within 2^-12 of half an ulp) are the ones a non-canonical split gets wrong
    {
        size_t n = 0, ties = 0;
        auto one = [&](float x) {
            uint16_t hi, lo, hi2, lo2;
            split2h(x, hi, lo);
            const float j = join2h(hi, lo);
            split2h(j, hi2, lo2);
            CHECK(hi2 == hi && lo2 == lo, "split2h(join2h) of the pair of %.9g: (%04x %04x) -> (%04x %04x)", x, hi, lo, hi2, lo2);
            const double tol = std::max(std::ldexp(std::fabs((double)x), -23), std::ldexp(1.0, -36));
            CHECK(std::fabs((double)j - (double)x) <= tol, "round trip of %.9g gives %.9g", x, j);
            n++;
        };
        for (int i = 0; i < 2000000; i++) {
            const double mag = std::exp2(-24.0 + uniform() * (std::log2(65504.0) + 24.0));
            one((float)(uniform() < 0.5 ? -mag : mag));
        }
        for (uint32_t h = 0x0400u; h < 0x7bffu; h += 7) {  // around the midpoints between neighbouring halves, both sides, a few fp32 steps
            const float v = pair_f16_value((uint16_t)h), w = pair_f16_value((uint16_t)(h + 1));
            float x = 0.5f * (v + w);
            for (int s = 0; s < 6; s++) { x = std::nextafterf(x, 0.0f); one(x); one(-x); ties++; }
            x = 0.5f * (v + w);
            for (int s = 0; s < 6; s++) { one(x); x = std::nextafterf(x, 1e30f); ties++; }
        }
        printf("split2h(join2h) identity: %zu values, %zu of them next to a tie\n", n, ties);
    }
    printf("f16 pair conv check: %s (%d failures)\n", g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
