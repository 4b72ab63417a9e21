// Host check of the fixed-geometry Stockham passes (csrc/fft_lds.h: fft_fixed_pass) against the run-time ones (fft_pass).
// Usage: fft_fixed_check N nfft nthreads in.f32 out.f32
//   in.f32:  nfft real frames of N floats (N = 512 or 400).  Each frame is packed z[n] = x[2n] + i x[2n+1] and transformed with both
//   forms of the passes, the way the STFT kernels run them (a thread is a value of tid, a pass is a barrier).
//   out.f32: rfft_post of the fixed-geometry result, nfft x (N/2 + 1) x (re, im).
//   exit 0 only if the two results are the same bits.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../speech_enhancement_mi_amd/csrc/fft_lds.h"

static cf2 *run_generic(cf2 *a, cf2 *b, int N2, int nfft, const cf2 *tw, int nth) {
    int rad[16];
    const int np = fft_plan(N2, rad);
    int Ns = 1;
    for (int p = 0; p < np; p++) {
        for (int tid = 0; tid < nth; tid++) {
            if (rad[p] == 5) fft_pass<5>(a, b, N2, N2, nfft, Ns, tw, tid, nth, 2);
            if (rad[p] == 4) fft_pass<4>(a, b, N2, N2, nfft, Ns, tw, tid, nth, 2);
            if (rad[p] == 2) fft_pass<2>(a, b, N2, N2, nfft, Ns, tw, tid, nth, 2);
        }
        Ns *= rad[p];
        cf2 *t = a; a = b; b = t;
    }
    return a;
}

template <int N2>
static cf2 *run_fixed(cf2 *a, cf2 *b, int nfft, const cf2 *tw, int nth) {
    for (int tid = 0; tid < nth; tid++) fft_fixed_pass<N2, 0>(a, b, nfft, tw, tid, nth);
    for (int tid = 0; tid < nth; tid++) fft_fixed_pass<N2, 1>(b, a, nfft, tw, tid, nth);
    for (int tid = 0; tid < nth; tid++) fft_fixed_pass<N2, 2>(a, b, nfft, tw, tid, nth);
    for (int tid = 0; tid < nth; tid++) fft_fixed_pass<N2, 3>(b, a, nfft, tw, tid, nth);
    return a;
}

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: fft_fixed_check N nfft nthreads in.f32 out.f32\n"); return 2; }
    const int N = atoi(argv[1]), nfft = atoi(argv[2]), nth = atoi(argv[3]), N2 = N / 2;
    if ((N != 512 && N != 400) || nfft <= 0 || nth <= 0) { fprintf(stderr, "bad argument\n"); return 2; }
    // the fixed plan is the plan fft_plan makes
    int rad[16];
    if (fft_plan(N2, rad) != kFixedPasses) { fprintf(stderr, "plan length\n"); return 1; }
    for (int p = 0; p < kFixedPasses; p++)
        if (rad[p] != fft_fixed_radix(N2, p)) { fprintf(stderr, "plan order\n"); return 1; }
    std::vector<float> x((size_t)nfft * N);
    FILE *fi = fopen(argv[4], "rb");
    if (!fi || fread(x.data(), sizeof(float), x.size(), fi) != x.size()) { fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    fclose(fi);
    std::vector<cf2> tw(N);  // the table of sig_chain_create
    for (int i = 0; i < N; i++) tw[i] = cf2{(float)cos(2.0 * M_PI * i / N), (float)-sin(2.0 * M_PI * i / N)};
    std::vector<cf2> ga((size_t)nfft * N2), gb(ga.size()), fa(ga.size()), fb(ga.size());
    for (int f = 0; f < nfft; f++)
        for (int n = 0; n < N2; n++) ga[(size_t)f * N2 + n] = fa[(size_t)f * N2 + n] = cf2{x[(size_t)f * N + 2 * n], x[(size_t)f * N + 2 * n + 1]};
    const cf2 *G = run_generic(ga.data(), gb.data(), N2, nfft, tw.data(), nth);
    const cf2 *Z = N == 512 ? run_fixed<256>(fa.data(), fb.data(), nfft, tw.data(), nth) : run_fixed<200>(fa.data(), fb.data(), nfft, tw.data(), nth);
    if (Z != fa.data()) { fprintf(stderr, "result buffer\n"); return 1; }
    if (memcmp(G, Z, sizeof(cf2) * ga.size()) != 0) { fprintf(stderr, "fixed and generic passes differ\n"); return 1; }
    std::vector<cf2> X((size_t)nfft * (N2 + 1));
    for (int f = 0; f < nfft; f++)
        for (int k = 0; k <= N2; k++) X[(size_t)f * (N2 + 1) + k] = rfft_post(Z + (size_t)f * N2, k, N2, tw.data());
    FILE *fo = fopen(argv[5], "wb");
    if (!fo || fwrite(X.data(), sizeof(cf2), X.size(), fo) != X.size()) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
    fclose(fo);
    return 0;
}
