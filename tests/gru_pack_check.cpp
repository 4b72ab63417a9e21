// Host check of the W_hh packing of the split-bf16 GRU step (csrc/gru_pack.h).  Usage: gru_pack_check H
//   1. gru_pack_index is a bijection of (gate, unit, k, plane) onto [0, 9 H^2);
//   2. every fragment - (unit group, k step, gate, plane): 32 units x 16 k - occupies 64 lanes x 16 bytes of contiguous memory, lane
//      32 (k half) + unit holding its 8 consecutive k in order, and the nine fragments of a k step follow each other;
//   3. the packed planes of seeded weights (and of a few special values) sum back to each weight exactly: hi + mid + lo == w.
// Exit status 0 when all three hold; the first violation is printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../speech_enhancement_mi_amd/csrc/gru_pack.h"

int main(int argc, char **argv) {
    const int H = argc > 1 ? atoi(argv[1]) : 64;
    if (H <= 0 || H % 32) { printf("H must be a positive multiple of 32\n"); return 2; }
    const size_t total = se::gru_pack_size(H);
    // 1. bijection
    std::vector<unsigned char> seen(total, 0);
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++)
                for (int p = 0; p < 3; p++) {
                    const size_t i = se::gru_pack_index(H, g, n, k, p);
                    if (i >= total) { printf("index out of range: g %d n %d k %d p %d -> %zu\n", g, n, k, p, i); return 1; }
                    if (seen[i]++) { printf("index hit twice: g %d n %d k %d p %d -> %zu\n", g, n, k, p, i); return 1; }
                }
    for (size_t i = 0; i < total; i++)
        if (!seen[i]) { printf("index %zu never written\n", i); return 1; }
    // 2. fragments: 512 elements (1 KB) each, in the order [unit group][k step][gate][plane]
    size_t frag = 0;
    for (int ng = 0; ng < H / 32; ng++)
        for (int ks = 0; ks < H / 16; ks++)
            for (int g = 0; g < 3; g++)
                for (int p = 0; p < 3; p++, frag++)
                    for (int lane = 0; lane < 64; lane++)
                        for (int e = 0; e < 8; e++) {
                            const int n = ng * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + e;
                            const size_t want = (frag * 64 + lane) * 8 + e, got = se::gru_pack_index(H, g, n, k, p);
                            if (got != want) { printf("fragment %zu lane %d element %d at %zu, expected %zu\n", frag, lane, e, got, want); return 1; }
                        }
    // 3. exact planes
    std::vector<float> w((size_t)3 * H * H);
    unsigned s = 2463534242u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffffff) / 8388608.0f - 1.0f; };  // 24 random bits in [-1, 1)
    for (auto &v : w) v = rnd() * 0.125f;
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.99999994f, 1.00000012f, 3.0e-5f, -7.5f, 255.99998f, 1.0f / 3.0f};
    for (size_t i = 0; i < sizeof(special) / sizeof(float); i++) w[i * 37 % w.size()] = special[i];
    std::vector<uint16_t> pk;
    se::gru_pack_whh(w.data(), H, pk);
    if (pk.size() != total) { printf("packed size %zu, expected %zu\n", pk.size(), total); return 1; }
    for (int g = 0; g < 3; g++)
        for (int n = 0; n < H; n++)
            for (int k = 0; k < H; k++) {
                const float x = w[((size_t)g * H + n) * H + k];
                const float hi = se::gru_pack_bf16_f32(pk[se::gru_pack_index(H, g, n, k, 0)]);
                const float mid = se::gru_pack_bf16_f32(pk[se::gru_pack_index(H, g, n, k, 1)]);
                const float lo = se::gru_pack_bf16_f32(pk[se::gru_pack_index(H, g, n, k, 2)]);
                // double holds the sum of three bf16 values of these magnitudes exactly, so this is an exact comparison
                if ((double)hi + (double)mid + (double)lo != (double)x) {
                    printf("planes of w[%d][%d][%d] = %.9g sum to %.9g\n", g, n, k, x, (double)hi + mid + lo);
                    return 1;
                }
            }
    printf("H %d: %zu elements, %zu fragments, bijection ok, fragments contiguous, planes exact\n", H, total, frag);
    return 0;
}
