// f16_pair_check.cpp - host check of the fp16 pair operand format (csrc/split_f16pair.h) and of its weight packers (csrc/gru_pack.h,
// pair_weight_matrix).  Plain C++: g++ -O2 -std=c++17 f16_pair_check.cpp && ./a.out [hidden].  Exit status 0 = every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

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

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static double uniform() {  // [0, 1)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}

// |join(split(x)) - x| <= max(2^-23 |x|, 2^-36)
static void round_trip(float x) {
    uint16_t hi, lo;
    split2h(x, hi, lo);
    const double back = (double)join2h(hi, lo), err = std::fabs(back - (double)x);
    const double tol = std::max(std::ldexp(std::fabs((double)x), -23), std::ldexp(1.0, -36));
    CHECK(err <= tol, "round trip of %.9g gives %.9g (error %.3g, allowed %.3g)", x, back, err, tol);
    CHECK(((hi >> 10) & 31) != 31 && ((lo >> 10) & 31) != 31, "split of %.9g is not finite (%04x %04x)", x, hi, lo);
}

int main(int argc, char **argv) {
    const int H = argc > 1 ? atoi(argv[1]) : 64;
    // ---- the fp16 conversion itself: every finite half survives a round trip, and the half-way points between neighbours
    // round to the even neighbour, their fp32 neighbours to the nearer one
    for (uint32_t h = 0; h < 0x7c00u; h++) {
        const float v = pair_f16_value((uint16_t)h);
        CHECK(pair_f16_bits(v) == h, "half %04x -> %.9g -> %04x", h, v, pair_f16_bits(v));
        CHECK(pair_f16_bits(-v) == (h | 0x8000u), "half -%04x", h);
        if (h + 1 < 0x7c00u) {
            const float w = pair_f16_value((uint16_t)(h + 1));
            CHECK(w > v, "halves %04x, %04x not ordered", h, h + 1);
            const float mid = 0.5f * (v + w);  // exact: 12 significant bits
            const uint16_t even = (h & 1u) ? (uint16_t)(h + 1) : (uint16_t)h;
            CHECK(pair_f16_bits(mid) == even, "tie between %04x and %04x went to %04x", h, h + 1, pair_f16_bits(mid));
            CHECK(pair_f16_bits(std::nextafterf(mid, 0.0f)) == h, "below the tie of %04x", h);
            CHECK(pair_f16_bits(std::nextafterf(mid, 1e30f)) == h + 1, "above the tie of %04x", h);
        }
    }
    CHECK(pair_f16_bits(65519.996f) == 0x7bffu && pair_f16_bits(65520.0f) == 0x7c00u, "rounding at the top of the range");
    // ---- split2h / join2h
    const float specials[] = {0.0f, -0.0f, 65504.0f, -65504.0f, 1e-8f, -1e-8f, 65503.99f, 6.1035156e-5f, 6.0e-5f, 5.9604645e-8f, 1.0f / 3.0f};
    for (float x : specials) round_trip(x);
    for (int e = -40; e <= 15; e++) { round_trip(std::ldexp(1.0f, e)); round_trip(-std::ldexp(1.0f, e)); if (e < 15) round_trip(std::ldexp(1.0f, e) * 1.9999999f); }  // (2^16 is beyond the range: clamped, below)
    for (int i = 0; i < 2000000; i++) {  // log-uniform magnitudes over 2^-30 .. 65504, both signs
        const double mag = std::exp2(-30.0 + uniform() * (std::log2(65504.0) + 30.0));
        round_trip((float)(uniform() < 0.5 ? -mag : mag));
    }
    {   // clamping: beyond the fp16 range the value is the clipped +-65504, never inf or NaN
        const float inf = std::numeric_limits<float>::infinity();
        const float big[] = {65504.01f, 65520.0f, 7e4f, 1e6f, 3e38f, inf};
        for (float x : big)
            for (float sgn : {1.0f, -1.0f}) {
                uint16_t hi, lo;
                split2h(sgn * x, hi, lo);
                CHECK(join2h(hi, lo) == sgn * 65504.0f, "clamp of %g gives %g", sgn * x, join2h(hi, lo));
            }
        uint16_t hi, lo;
        split2h(std::numeric_limits<float>::quiet_NaN(), hi, lo);
        CHECK(std::isfinite(join2h(hi, lo)), "NaN operand is not finite after the split");
    }
    // ---- weight planes (2^11 hi, lo, hi): matrix layout [3][n] and the packed W_hh image at the indices the step kernel reads
    std::vector<float> w((size_t)3 * H * H);
    for (float &x : w) {
        const double mag = std::exp2(-20.0 + uniform() * 23.9);  // up to just under 2^4, the guard's limit
        x = (float)(uniform() < 0.5 ? -mag : mag);
    }
    w[0] = 15.999f; w[1] = -15.999f; w[2] = 0.0f;
    std::vector<uint16_t> planes(3 * w.size()), pk;
    pair_weight_matrix(w.data(), w.size(), planes.data());
    gru_pack_whh_pair(w.data(), H, pk);
    CHECK(pk.size() == gru_pack_size(H), "packed size");
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++) {
                const size_t i = ((size_t)g * H + n) * H + k;
                uint16_t hi, lo;
                split2h(w[i], hi, lo);
                const uint16_t p0 = planes[i], p1 = planes[w.size() + i], p2 = planes[2 * w.size() + i];
                CHECK(p2 == hi && p1 == lo, "planes 1, 2 of weight %zu", i);
                CHECK(pair_f16_value(p0) == 2048.0f * pair_f16_value(hi), "plane 0 of weight %zu: %g vs 2048 * %g", i, pair_f16_value(p0), pair_f16_value(hi));
                CHECK(((p0 >> 10) & 31) != 31, "2^11 hi of %g overflows", w[i]);
                // what the three MFMA terms reconstruct with a = 1: (W0 + W1) * 2^-11 = hi + lo 2^-11
                const double back = ((double)pair_f16_value(p0) + (double)pair_f16_value(p1)) / 2048.0;
                CHECK(std::fabs(back - (double)w[i]) <= std::max(std::ldexp(std::fabs((double)w[i]), -23), std::ldexp(1.0, -36)), "weight %zu: %.9g vs %.9g", i, back, w[i]);
                CHECK(pk[gru_pack_index(H, g, n, k, 0)] == p0 && pk[gru_pack_index(H, g, n, k, 1)] == p1 && pk[gru_pack_index(H, g, n, k, 2)] == p2,
                      "packed W_hh planes at gate %d unit %d k %d", g, n, k);
            }
    printf("f16 pair check, H = %d: %s (%d failures)\n", H, g_fail ? "FAILED" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
