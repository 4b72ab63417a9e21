// io_fused.hip.h - the two ends of the CRN engine's segment with the neighbouring elementwise kernel folded into the FFT kernel:
//
//   k_stft_feat   k_stft of all microphones of a stream + k_featurize_p: the spectra stay in LDS, the feature octet
//                 [mag_0..M-1, dphi_1..M-1, 0...] goes straight into the P layout of the encoder's ring slot, and only microphone 0's
//                 spectrum (which the mask multiplies later) is written out.  Removes the write of M-1 spectra and featurize's read.
//   k_mask_istft  k_final_mask_p + k_istft: last gLN, decompress_cIRM and the complex multiply form the masked spectrum in LDS, then
//                 irfft_pre, the passes, the window and the overlap-add as in k_istft.  Removes the masked spectrum's write and read.
//
// The arithmetic is that of the kernels they replace, expression for expression (rfft_post / irfft_pre / the passes of fft_lds.h, the
// feature and mask expressions of conv_p.hip.h): tests/test_gpu_io_fused.py asks for the same bits as the four-kernel route (SE_IO_FUSE=0).
#pragma once
#include <hip/hip_runtime.h>

#include "conv_p_args.h"
#include "norm.hip.h"
#include "stft.hip.h"
#ifdef SE_AUX_KERNELS
#include "conv_p.hip.h"  // split_store8
#endif

namespace se {

// k_stft_feat: a workgroup owns kFeatFrames frames of all M microphones of one stream (grid: streams x ceil(T / kFeatFrames)); T = 21 is
// seven full slices.  The kernel's time is vector-ALU time, and most of it is the feature stage (per bin three rfft_post, sqrt, atan and
// eight three-way bf16 splits, as in k_featurize_p), so the workgroup is sized for THAT stage: 3 x 256 bins are exactly two trips of
// 384 threads, and the three Nyquist bins are a third trip of one wave.  The passes (M = 3: nine 256-point transforms, 576 radix-4
// butterflies) then take one and a half trips.  LDS at n_fft = 512, hop = 160: 3 x 832 signal floats + tables + 2 x 9 x 2 KB = 52 KB,
// three workgroups (18 waves) per CU.
constexpr int kFeatFrames = 3;
constexpr int kFeatThreads = 384;
constexpr int kFeatMaxM = 4;  // the octet has eight lanes: M magnitudes + M - 1 phase differences

struct StftFeatArgs {
    StftArgs s;          // as k_stft (rows are streams: Lrow / offrow / zero fill outside [0, L)); spec = microphone 0 only, sR = its stream stride
    uint4 *feat;         // P[b][0][pl][t][f] of the ring slot
    long feat_stream;    // uint4 per stream
    int atan2_phase;
};

// LDS: sig[M][(kFeatFrames-1)*hop + N] | win[N] | tw[N] (cf2) | bufA[M*kFeatFrames*N/2] | bufB[...]
inline size_t stft_feat_lds_bytes(int hop, int N, int M) {
    return sizeof(float) * ((size_t)M * ((kFeatFrames - 1) * hop + N) + N) + sizeof(cf2) * ((size_t)N + (size_t)M * kFeatFrames * N);
}

struct MaskIstftArgs {
    MaskPArgs m;  // as k_final_mask_p (out unused)
    IstftArgs i;  // as k_istft (spec unused); rows are streams
};

// k_mask_istft: one workgroup per stream holds all T frames (at T = 21, n_fft = 512: 1344 butterflies per pass, three per thread).
// LDS: win[N] | tw[N] (cf2) | bufA[T*N/2] | bufB[T*(N/2+1)] - bufB first holds the masked spectrum; the windowed frames replace the
// transforms' result in place.
inline size_t mask_istft_lds_bytes(int T, int N) {
    return sizeof(float) * (size_t)N + sizeof(cf2) * ((size_t)N + (size_t)T * (N / 2) + (size_t)T * (N / 2 + 1));
}

#ifdef SE_AUX_KERNELS
template <int NFFT, int PL>
__global__ __launch_bounds__(kFeatThreads) void k_stft_feat(StftFeatArgs fa) {
    extern __shared__ __align__(16) unsigned char smem[];
    const StftArgs &a = fa.s;
    const int N = NFFT ? NFFT : a.plan.N, N2 = N / 2, K = a.K, T = a.T, F = N2 + 1, pad = N / 2, M = a.M;
    const int SL = (kFeatFrames - 1) * a.hop + N;
    float *sig = reinterpret_cast<float *>(smem);
    float *win = sig + M * SL;
    cf2 *tw = reinterpret_cast<cf2 *>(win + N);
    cf2 *bufA = tw + N;
    cf2 *bufB = bufA + M * kFeatFrames * N2;
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const int t0 = blockIdx.y * kFeatFrames, nf = min(kFeatFrames, T - t0);
    const long seg_first = a.offrow ? a.offrow[b] + a.off : a.off;
    const long Lr = a.Lrow ? min(a.Lrow[b], a.L) : a.L;
    const int nsl = (nf - 1) * a.hop + N;  // samples of the padded segment that the slice's frames cover, from t0 * hop
    for (int m = 0; m < M; m++) {
        const float *src = a.src + (long)b * a.strideB + (long)m * a.strideM;
        for (int i = tid; i < nsl; i += nth) {
            const int p = t0 * a.hop + i;
            const long k = (long)p - pad + seg_first;
            sig[m * SL + i] = (p >= pad && p < pad + K && k >= 0 && k < Lr) ? src[k] : 0.0f;
        }
    }
    for (int i = tid; i < N; i += nth) { win[i] = a.window[i]; tw[i] = a.tw[i]; }
    __syncthreads();
    // transform m * nf + f = frame t0 + f of microphone m
    for (int i = tid; i < M * nf * N2; i += nth) {
        const int q = i / N2, n = i - q * N2, m = q / nf, f = q - m * nf;
        const float *s = sig + m * SL + f * a.hop + 2 * n;
        bufA[i] = cf2{win[2 * n] * s[0], win[2 * n + 1] * s[1]};
    }
    __syncthreads();
    const cf2 *Z = fft_run_t<NFFT>(bufA, bufB, a.plan, M * nf, tw);
    const long TF = (long)T * F;
    for (int i = tid; i < nf * F; i += nth) {
        // bins [0, N2) of every frame first, the Nyquist bins last: full trips where the count of bins allows it
        const int f = i < nf * N2 ? i / N2 : i - nf * N2, k = i < nf * N2 ? i - f * N2 : N2;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float ang0 = 0.0f;
#pragma unroll
        for (int m = 0; m < kFeatMaxM; m++) {
            if (m >= M) continue;
            const cf2 v = rfft_post(Z + (m * nf + f) * N2, k, N2, tw);
            if (m == 0) a.spec[(long)b * a.sR + (long)(t0 + f) * a.sT + (long)k * a.sF] = v;
            const float mag = sqrtf(v.x * v.x + v.y * v.y + 1e-10f);
            const float ang = fa.atan2_phase ? atan2f(v.y, v.x) : atanf(v.y / (v.x + kEps) + kEps);
            if (m == 0) ang0 = ang;
#pragma unroll
            for (int c = 0; c < 8; c++) {  // (static register indices)
                if (c == m) o[c] = mag;
                if (m > 0 && c == M + m - 1) o[c] = ang0 - ang;
            }
        }
        split_store8<PL>(o, fa.feat + (long)b * fa.feat_stream + (long)(t0 + f) * F + k, TF);
    }
}

template <int NFFT>
__global__ __launch_bounds__(kFftThreads) void k_mask_istft(MaskIstftArgs ma) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float sm[2];
    const MaskPArgs &m = ma.m;
    const IstftArgs &a = ma.i;
    const int N = NFFT ? NFFT : a.plan.N, N2 = N / 2, K = a.K, T = a.T, F = N2 + 1, pad = N / 2;
    float *win = reinterpret_cast<float *>(smem);
    cf2 *tw = reinterpret_cast<cf2 *>(win + N);
    cf2 *bufA = tw + N;
    cf2 *bufB = bufA + T * N2;
    const int b = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    for (int i = tid; i < N; i += nth) { win[i] = a.window[i]; tw[i] = a.tw[i]; }
    float mean, inv;
    slab_mean_inv(m.st, b, sm, mean, inv);  // (contains a barrier)
    // masked spectrum of every frame: the expression of k_final_mask_p
    {
        cf2 *ms = bufB;
        const float *y = m.y + (long)b * m.y_stream;
        const float w0 = m.nw[0], w1 = m.nw[1], b0 = m.nb[0], b1 = m.nb[1];
        for (int i = tid; i < T * F; i += nth) {
            const int t = i / F, f = i - t * F;
            const float *p = y + ((long)t * m.Fh + (f >> 1)) * 8 + (f & 1);
            const float mr = decompress_cirm((p[0] - mean) * inv * w0 + b0);
            const float mi = decompress_cirm((p[2] - mean) * inv * w1 + b1);
            const cf2 n = m.spec[(long)b * m.sB + (long)t * m.sT + (long)f * m.sF];
            ms[i] = cf2{mr * n.x - mi * n.y, mi * n.x + mr * n.y};
        }
        __syncthreads();
        for (int i = tid; i < T * N2; i += nth) {
            const int f = i / N2, k = i - f * N2;
            const cf2 *s = ms + f * F;
            cf2 xk = s[k], xn = s[N2 - k];
            if (k == 0) { xk.y = 0; xn.y = 0; }  // C2R ignores Im of DC / Nyquist
            bufA[i] = irfft_pre(xk, xn, k, tw);
        }
        __syncthreads();
    }
    cf2 *R = fft_run_t<NFFT>(bufA, bufB, a.plan, T, tw);
    float *frames = reinterpret_cast<float *>(R);  // frame t at frames + t * N: element i of R becomes samples 2n, 2n+1 of its frame
    const float invN2 = 1.0f / (float)N2;
    for (int i = tid; i < T * N2; i += nth) {
        const int n = i % N2;
        const cf2 r = R[i];
        frames[2 * i] = (r.x * invN2) * win[2 * n];
        frames[2 * i + 1] = (-r.y * invN2) * win[2 * n + 1];
    }
    __syncthreads();
    for (int i = tid; i < K; i += nth) {
        const int pos = pad + i;
        int t0 = (pos - N + a.hop) / a.hop;  // ceil((pos-N+1)/hop)
        if (t0 < 0) t0 = 0;
        int t1 = pos / a.hop;
        if (t1 > T - 1) t1 = T - 1;
        float s = 0.0f;
        for (int t = t0; t <= t1; t++) s += frames[t * N + (pos - t * a.hop)];
        a.wav[(long)b * a.wav_ld + i] = s / a.env[i];
    }
}
#endif  // SE_AUX_KERNELS

}  // namespace se
