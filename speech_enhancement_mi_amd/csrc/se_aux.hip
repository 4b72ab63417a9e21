// se_aux.hip - the kernels of the path that do COMPLEX arithmetic (LDS FFTs of the STFT / iSTFT, FullSubNet's mask application),
// compiled as their own translation unit with -fno-slp-vectorize.
//
// Why: with SLP vectorisation hipcc turns the (re, im) float pairs of these kernels into packed-FP32 VALU instructions
// with operand swizzles (v_pk_mul_f32 / v_pk_fma_f32 ... op_sel:[1,1], neg_lo/neg_hi, v_pk_mov_b32).  On MI355X those
// kernels returned wrong values - transiently, in 35 % of the launches - whenever their waves shared a SIMD with waves of
// this engine's MFMA kernels launched from another stream (signal / window / twiddle tables in LDS intact,
// a redundant re-execution of one radix-4 pass inside the kernel differs, scalar-FMA and integer LDS victims never fail,
// plain op_sel_hi-only packed ops as in k_conv_small never failed either).  Built without SLP the same kernels contain
// no packed-FP32 instruction, cost the same time (STFT 56 vs 57 us) and are exact under co-execution (0 of 800 launches
// differed; tests/test_gpu_parity.py::test_fft_kernels_exact_under_coexecution and tests/test_isa_inventory.py keep it so).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#define SE_AUX_KERNELS 1
#include "../../include/se_engine.h"
#include "fft_lds.h"
#include "norm.hip.h"
#include "stft.hip.h"
#include "fsn_mask.hip.h"
#include "io_fused.hip.h"
#include "sig_chain.h"

namespace se {

// n_fft = 512 and 400 have passes with compile-time geometry (fft_lds.h); every other size runs the run-time plan
void launch_k_stft(dim3 grid, size_t lds, hipStream_t st, const StftArgs &a) {
    if (a.plan.N == 512) hipLaunchKernelGGL(k_stft<512>, grid, dim3(kFftThreads), lds, st, a);
    else if (a.plan.N == 400) hipLaunchKernelGGL(k_stft<400>, grid, dim3(kFftThreads), lds, st, a);
    else hipLaunchKernelGGL(k_stft<0>, grid, dim3(kFftThreads), lds, st, a);
}

void launch_k_istft(dim3 grid, size_t lds, hipStream_t st, const IstftArgs &a) {
    if (a.plan.N == 512) hipLaunchKernelGGL(k_istft<512>, grid, dim3(kFftThreads), lds, st, a);
    else if (a.plan.N == 400) hipLaunchKernelGGL(k_istft<400>, grid, dim3(kFftThreads), lds, st, a);
    else hipLaunchKernelGGL(k_istft<0>, grid, dim3(kFftThreads), lds, st, a);
}

void launch_k_overlap_avg(dim3 grid, hipStream_t st, const float *yseg, float *out, int Nseg, int K, long L, long skip, const long *Lrow,
                          const long *skiprow) {
    hipLaunchKernelGGL(k_overlap_avg, grid, dim3(256), 0, st, yseg, out, Nseg, K, L, skip, Lrow, skiprow);
}

void launch_k_fsn_mask(dim3 grid, hipStream_t st, const FsnMaskArgs &a) { hipLaunchKernelGGL(k_fsn_mask, grid, dim3(256), 0, st, a); }

void aux_set_fft_lds(int stft_bytes, int istft_bytes) {
    // engines / signal handles of different STFT sizes share the kernels: the opt-in only ever grows
    // (a geometry whose segment does not fit the 160 KB of LDS - FullSubNet's train=True engine with one N*T-frame "segment" -
    // never launches these kernels and must not poison the opt-in of the others)
    static int cur_stft = 0, cur_istft = 0;
    const int kMaxLds = 160 * 1024;
    if (stft_bytes <= kMaxLds && stft_bytes > cur_stft) cur_stft = stft_bytes;
    if (istft_bytes <= kMaxLds && istft_bytes > cur_istft) cur_istft = istft_bytes;
    stft_bytes = cur_stft; istft_bytes = cur_istft;
    for (const void *k : {reinterpret_cast<const void *>(k_stft<512>), reinterpret_cast<const void *>(k_stft<400>), reinterpret_cast<const void *>(k_stft<0>)})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, stft_bytes);
    for (const void *k : {reinterpret_cast<const void *>(k_istft<512>), reinterpret_cast<const void *>(k_istft<400>), reinterpret_cast<const void *>(k_istft<0>)})
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, istft_bytes);
}

// ---- the signal chain (sig_chain.h) ----
int sig_chain_create(SigChain &s, int n_fft, int win, int hop, int K, int device, std::string &err) {
    s = SigChain{};
    if (n_fft <= 0 || n_fft % 2 || win <= 0 || win > n_fft || hop <= 0 || K <= 0 || K % hop) { err = "bad STFT geometry"; return SE_ERR_ARG; }
    s.device = device; s.N = n_fft; s.win = win; s.hop = hop; s.K = K; s.T = 1 + K / hop; s.F = n_fft / 2 + 1;
    s.plan.N = n_fft;
    s.plan.npass = fft_plan(n_fft / 2, s.plan.radices);
    if (!s.plan.npass || s.plan.npass > kMaxRadices) { err = "n_fft must factor into 2s and 5s"; return SE_ERR_ARG; }
    if (hipSetDevice(device) != hipSuccess) { err = "hipSetDevice failed"; return SE_ERR_HIP; }
    // tables: hamming(win) centred in n_fft (torch.stft), twiddles, overlap-add envelope
    const int N = n_fft, T = s.T;
    std::vector<float> w(N, 0.0f), tw(2 * (size_t)N), env(K, 0.0f);
    const int left = (N - win) / 2;
    for (int i = 0; i < win; i++) w[left + i] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * i / win));
    for (int i = 0; i < N; i++) { tw[2 * i] = (float)cos(2.0 * M_PI * i / N); tw[2 * i + 1] = (float)-sin(2.0 * M_PI * i / N); }
    for (int i = 0; i < K; i++) {
        const int pos = N / 2 + i;
        float sum = 0;
        for (int t = 0; t < T; t++) { const int n = pos - t * hop; if (n >= 0 && n < N) sum += w[n] * w[n]; }
        env[i] = sum;
    }
    auto up = [](float *&d, const std::vector<float> &h) {
        return hipMalloc(reinterpret_cast<void **>(&d), h.size() * sizeof(float)) == hipSuccess &&
               hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(s.window, w) || !up(s.tw, tw) || !up(s.env, env)) { sig_chain_destroy(s); err = "STFT table upload failed"; return SE_ERR_HIP; }
    aux_set_fft_lds((int)stft_lds_bytes(K, N), (int)istft_lds_bytes(T, N));
    return SE_OK;
}

void sig_chain_destroy(SigChain &s) {
    if (!s.window && !s.tw && !s.env) return;
    (void)hipSetDevice(s.device);
    for (float **p : {&s.window, &s.tw, &s.env}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

hipError_t sig_stft(const SigChain &s, const float *src, long strideB, long strideM, int M, long off, long Lsrc, SigRows rows, int nrows, cf2 *spec,
                    long sR, long sT, long sF, hipStream_t st, int nseg, long seg_off, long seg_spec) {
    StftArgs a{};
    a.src = src; a.strideB = strideB; a.strideM = strideM; a.M = M; a.off = off; a.L = Lsrc;
    a.K = s.K; a.T = s.T; a.F = s.F; a.hop = s.hop;
    a.spec = spec; a.sR = sR; a.sT = sT; a.sF = sF;
    a.window = s.window; a.tw = reinterpret_cast<const cf2 *>(s.tw); a.plan = s.plan;
    a.seg_off = seg_off; a.seg_spec = seg_spec;
    a.Lrow = rows.len; a.offrow = rows.off0;
    launch_k_stft(dim3(nrows, nseg), stft_lds_bytes(s.K, s.N), st, a);
    return hipGetLastError();
}

hipError_t sig_istft(const SigChain &s, const cf2 *spec, long sR, long sT, long sF, int nrows, float *wav, long wav_ld, hipStream_t st, int nseg,
                     long seg_spec, long seg_wav) {
    IstftArgs a{};
    a.spec = spec; a.sR = sR; a.sT = sT; a.sF = sF; a.K = s.K; a.T = s.T; a.F = s.F; a.hop = s.hop;
    a.wav = wav; a.wav_ld = wav_ld; a.window = s.window; a.env = s.env; a.tw = reinterpret_cast<const cf2 *>(s.tw); a.plan = s.plan;
    a.seg_spec = seg_spec; a.seg_wav = seg_wav;
    launch_k_istft(dim3(nrows, nseg), istft_lds_bytes(s.T, s.N), st, a);
    return hipGetLastError();
}

// ---- the fused ends (io_fused.hip.h) ----
namespace {

constexpr int kLdsMax = 160 * 1024, kLdsStatic = 256;

template <int NFFT>
void stft_feat_instances(const void **k) {
    k[0] = reinterpret_cast<const void *>(k_stft_feat<NFFT, 1>);
    k[1] = reinterpret_cast<const void *>(k_stft_feat<NFFT, 2>);
    k[2] = reinterpret_cast<const void *>(k_stft_feat<NFFT, 3>);
}

// dynamic-LDS opt-in of every instance: hipFuncSetAttribute is per device, so once per thread and device (as train_conv_attributes)
void io_fused_attributes() {
    static thread_local int done_dev = -1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (done_dev == dev) return;
    const void *k[12];
    stft_feat_instances<512>(k);
    stft_feat_instances<400>(k + 3);
    stft_feat_instances<0>(k + 6);
    k[9] = reinterpret_cast<const void *>(k_mask_istft<512>);
    k[10] = reinterpret_cast<const void *>(k_mask_istft<400>);
    k[11] = reinterpret_cast<const void *>(k_mask_istft<0>);
    // (k_mask_istft also has a few static bytes: kLdsStatic below the chip's 160 KB, as sig_io_fused_fits assumes)
    for (int i = 0; i < 12; i++) (void)hipFuncSetAttribute(k[i], hipFuncAttributeMaxDynamicSharedMemorySize, i < 9 ? kLdsMax : kLdsMax - kLdsStatic);
    (void)hipGetLastError();
    done_dev = dev;
}

template <int NFFT>
void launch_stft_feat(int PL, dim3 grid, size_t lds, hipStream_t st, const StftFeatArgs &a) {
    if (PL == 1) hipLaunchKernelGGL((k_stft_feat<NFFT, 1>), grid, dim3(kFeatThreads), lds, st, a);
    else if (PL == 2) hipLaunchKernelGGL((k_stft_feat<NFFT, 2>), grid, dim3(kFeatThreads), lds, st, a);
    else hipLaunchKernelGGL((k_stft_feat<NFFT, 3>), grid, dim3(kFeatThreads), lds, st, a);
}

}  // namespace

bool sig_io_fused_fits(const SigChain &s, int M) {
    return M >= 1 && M <= kFeatMaxM && stft_feat_lds_bytes(s.hop, s.N, M) <= (size_t)kLdsMax && mask_istft_lds_bytes(s.T, s.N) + kLdsStatic <= (size_t)kLdsMax;
}

hipError_t sig_stft_feat(const SigChain &s, const float *src, long strideB, long strideM, int M, long off, long Lsrc, SigRows rows, int nstreams,
                         cf2 *spec0, long sB, long sT, long sF, uint4 *feat, long feat_stream, int PL, int atan2_phase, hipStream_t st) {
    if (!sig_io_fused_fits(s, M) || PL < 1 || PL > 3) return hipErrorInvalidValue;
    StftFeatArgs fa{};
    StftArgs &a = fa.s;
    a.src = src; a.strideB = strideB; a.strideM = strideM; a.M = M; a.off = off; a.L = Lsrc;
    a.K = s.K; a.T = s.T; a.F = s.F; a.hop = s.hop;
    a.spec = spec0; a.sR = sB; a.sT = sT; a.sF = sF;
    a.window = s.window; a.tw = reinterpret_cast<const cf2 *>(s.tw); a.plan = s.plan;
    a.Lrow = rows.len; a.offrow = rows.off0;
    fa.feat = feat; fa.feat_stream = feat_stream; fa.atan2_phase = atan2_phase;
    io_fused_attributes();
    const dim3 grid(nstreams, (s.T + kFeatFrames - 1) / kFeatFrames);
    const size_t lds = stft_feat_lds_bytes(s.hop, s.N, M);
    if (s.N == 512) launch_stft_feat<512>(PL, grid, lds, st, fa);
    else if (s.N == 400) launch_stft_feat<400>(PL, grid, lds, st, fa);
    else launch_stft_feat<0>(PL, grid, lds, st, fa);
    return hipGetLastError();
}

hipError_t sig_mask_istft(const SigChain &s, const MaskPArgs &m, int nstreams, float *wav, long wav_ld, hipStream_t st) {
    if (!sig_io_fused_fits(s, 1)) return hipErrorInvalidValue;
    MaskIstftArgs ma{};
    ma.m = m;
    IstftArgs &a = ma.i;
    a.K = s.K; a.T = s.T; a.F = s.F; a.hop = s.hop;
    a.wav = wav; a.wav_ld = wav_ld; a.window = s.window; a.env = s.env; a.tw = reinterpret_cast<const cf2 *>(s.tw); a.plan = s.plan;
    io_fused_attributes();
    const size_t lds = mask_istft_lds_bytes(s.T, s.N);
    if (s.N == 512) hipLaunchKernelGGL(k_mask_istft<512>, dim3(nstreams), dim3(kFftThreads), lds, st, ma);
    else if (s.N == 400) hipLaunchKernelGGL(k_mask_istft<400>, dim3(nstreams), dim3(kFftThreads), lds, st, ma);
    else hipLaunchKernelGGL(k_mask_istft<0>, dim3(nstreams), dim3(kFftThreads), lds, st, ma);
    return hipGetLastError();
}

}  // namespace se
