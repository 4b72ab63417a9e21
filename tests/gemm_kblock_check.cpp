// gemm_kblock_check.cpp - host check of the K-blocked pair operands of k_gemm_p<2, kF16Pair, true> (csrc/gemm_kblock.h).
// Plain C++: g++ -O2 -std=c++17 gemm_kblock_check.cpp && ./a.out.  Exit status 0 = every check held.
//   1. the K-blocked weight image holds planes (w_lo, w_hi) of pair_weight_matrix2 at every index the kernel's LDS-DMA reads, and
//      nothing else (K = 32, 512, 2176; N with and without a 128-column tail);
//   2. the LDS swizzle is a bijection per 1-KB run (one wave instruction: 8 rows x 8 pieces), and staging + fragment read together
//      return the fragment of the plane-major kernel: 8 consecutive k of the right plane;
//   3. a brute-force bank model of ds_read_b128 (four 16-lane groups, 64 banks of 4 bytes) shows no conflict for both K steps, both
//      lane halves, both planes, both row offsets of a wave and every wave position.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../speech_enhancement_mi_amd/csrc/gemm_kblock.h"

using namespace se;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (failures < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } \
            failures++;                                    \
        }                                                  \
    } while (0)

// What one ring stage of k_gemm_p receives for an operand of `rows_tile` rows (256 for A, 128 for W) at chunk kc, as the kernel's
// staging addresses it: LDS piece s (lane-linear) <- source piece (row r clamped, 2 K8 pieces per row, + 8 kc, kblock_lds_slot).
static std::vector<long> stage_sources(int rows_tile, int row0, int rows, int K, int kc) {
    const long K8 = K / 8;
    std::vector<long> src(rows_tile * 8);
    for (int s = 0; s < rows_tile * 8; s++) {
        const int row = s >> 3;
        const long r = std::min(row0 + row, rows - 1);
        src[s] = r * 2 * K8 + kblock_lds_slot(row, s & 7) + 8L * kc;  // in 16-byte pieces
    }
    return src;
}

static void check_weight_image(int N, int K, std::mt19937 &rng) {
    std::uniform_real_distribution<float> d(-2.0f, 2.0f);
    const size_t n = (size_t)N * K;
    std::vector<float> w(n);
    for (auto &x : w) x = d(rng);
    w[0] = 0.0f; w[n - 1] = -0.0f; w[n / 2] = 1e-6f; w[n / 3] = 15.9f;
    std::vector<uint16_t> planes(2 * n), kb(2 * n, 0xdead);
    pair_weight_matrix2(w.data(), n, planes.data());
    pair_weight_matrix2_kblock(w.data(), N, K, kb.data());
    // every element of the image is one (row, k, plane), each exactly once
    std::vector<char> seen(2 * n, 0);
    for (long r = 0; r < N; r++)
        for (long k = 0; k < K; k++)
            for (int p = 0; p < 2; p++) {
                const long i = kblock_index(r, K, k, p);
                CHECK(i >= 0 && i < (long)(2 * n) && !seen[i], "index N %d K %d r %ld k %ld p %d -> %ld", N, K, r, k, p, i);
                if (i >= 0 && i < (long)(2 * n)) seen[i] = 1;
                CHECK(kb[i] == planes[(size_t)p * n + r * K + k], "value N %d K %d r %ld k %ld p %d", N, K, r, k, p);
            }
    // through the kernel's eyes: every column tile, every chunk; the fragment of (row, ks, half, plane) is 8 consecutive k of plane-major
    for (int n0 = 0; n0 < N; n0 += 128)
        for (int kc = 0; kc < K / 32; kc++) {
            const std::vector<long> src = stage_sources(128, n0, N, K, kc);
            for (int row = 0; row < 128; row++)
                for (int ks = 0; ks < 2; ks++)
                    for (int half = 0; half < 2; half++)
                        for (int p = 0; p < 2; p++) {
                            const unsigned byte = kblock_frag_byte(row, ks, half, p);
                            CHECK(byte % 16 == 0 && byte / 16 < 128 * 8, "fragment offset out of the image");
                            const long piece = src[byte / 16];
                            CHECK(piece >= 0 && (piece + 1) * 8 <= (long)(2 * n), "source piece outside the buffer: N %d K %d", N, K);
                            const long r = std::min(n0 + row, N - 1), k = 32L * kc + 16 * ks + 8 * half;
                            for (int e = 0; e < 8; e++)
                                CHECK(kb[piece * 8 + e] == planes[(size_t)p * n + r * K + k + e], "fragment N %d K %d row %d kc %d ks %d half %d p %d", N, K, n0 + row, kc, ks, half, p);
                        }
        }
}

static void check_swizzle() {
    for (int run = 0; run < 32; run++) {  // a 256-row image is 32 runs of 1 KB = 8 rows x 8 slots
        std::set<int> got;
        for (int lane = 0; lane < 64; lane++) {
            const int s = run * 64 + lane, row = s >> 3;
            const int piece = kblock_lds_slot(row, s & 7);
            CHECK(piece >= 0 && piece < 8, "piece out of the line");
            got.insert(row * 8 + piece);
            CHECK(kblock_lds_slot(row, piece) == (s & 7), "the XOR is not its own inverse at row %d", row);
        }
        CHECK(got.size() == 64 && *got.begin() == run * 64 && *got.rbegin() == run * 64 + 63, "run %d is no bijection onto its 8 whole lines", run);
    }
}

// ds_read_b128: lane groups of 16, banks (a / 4) mod 64; conflict = two lanes of a group on one bank with different addresses
static void check_banks() {
    static const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                      {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int wrow = 0; wrow < 256; wrow += 64)      // wave row offsets wm (A) / wn (W: 0, 64)
        for (int i = 0; i < 2; i++)                 // row tile of the wave
            for (int ks = 0; ks < 2; ks++)
                for (int p = 0; p < 2; p++)
                    for (int g = 0; g < 4; g++) {
                        long owner[64];
                        for (auto &o : owner) o = -1;
                        for (int j = 0; j < 16; j++) {
                            const int lane = groups[g][j], half = lane >> 5, l31 = lane & 31;
                            const unsigned a = kblock_frag_byte(wrow + 32 * i + l31, ks, half, p);
                            for (int d = 0; d < 4; d++) {
                                const int bank = (a / 4 + d) % 64;
                                CHECK(owner[bank] < 0 || owner[bank] == (long)a, "bank conflict: rows %d+ ks %d plane %d group %d bank %d", wrow + 32 * i, ks, p, g, bank);
                                owner[bank] = a;
                            }
                        }
                    }
    // the kernel takes plane 1 at plane 0 + a per-lane constant, and row tile 1 at + 4096 bytes
    for (int row = 0; row < 256; row++)
        for (int ks = 0; ks < 2; ks++)
            for (int half = 0; half < 2; half++) {
                const unsigned dpl = kblock_frag_byte(row & 31, 0, 0, 1) - kblock_frag_byte(row & 31, 0, 0, 0);
                CHECK(kblock_frag_byte(row, ks, half, 0) + dpl == kblock_frag_byte(row, ks, half, 1), "plane offset at row %d", row);
                if (row + 32 < 256) CHECK(kblock_frag_byte(row, ks, half, 0) + 4096 == kblock_frag_byte(row + 32, ks, half, 0), "row tile offset at row %d", row);
            }
}

int main() {
    std::mt19937 rng(5);
    for (int K : {32, 512, 2176})
        for (int N : {128, 384, 200, 1}) check_weight_image(N, K, rng);  // whole tiles; a 72-column tail; a single row
    check_swizzle();
    check_banks();
    // the A side of the same staging: a 256-row tile with an M tail (840 rows: 72 in the last tile) stays inside the buffer
    for (int K : {32, 512, 2176})
        for (int m0 = 0; m0 < 840; m0 += 256)
            for (int kc : {0, K / 32 - 1})
                for (long piece : stage_sources(256, m0, 840, K, kc)) CHECK(piece >= 0 && piece < 840L * K / 4, "A piece outside the buffer");
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("gemm_kblock_check: weight images, swizzle bijection and bank model hold\n");
    return 0;
}
