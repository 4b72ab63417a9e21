// se_gbf.hip - the beamforming head of GeneralBeamformer (reference GeneralBeamformer.py:336-373) behind se_gbf_* (include/se_engine.h).
//
// The U-Net in front of it runs on the training kernels (se_train_conv_w / gln / skip); the two GRUs run on se_train_gru_pseq_fwd.
// Layout: S = N segments x B utterances, segment-major, as in train_net.CRNFunction.  Three launches, all fp32 arithmetic with double
// statistics, no atomics, every reduction in a fixed order that does not depend on S (bit-reproducible, chunk-independent):
//
//   k_gbf_psd  one workgroup per stream s.  Per bin: the complex 3x3 filter of the interleaved noisy plane (the unfold of
//              GeneralBeamformer.py:345), S_m / N_m, Phi = Re(S S^H), written straight into the GRU input rows [B][F][Nc][T][16]; then
//              ln_S / ln_N (gLN over F*T*9, weight per f*T + t) in place: mean, then sum (x - mean)^2, then normalise.  Each thread
//              only ever re-reads the rows it wrote itself.
//   k_gbf_seq  one workgroup per (s, f) sequence.  fc_output_layer (H -> 9) of both GRU models as wave dot products (lanes over H,
//              xor-butterfly reduction), ReLU, SequenceModel.norm (gLN over T x 9, per-feature weight), Phi = Phi_S * Phi_N.
//   k_gbf_bf   one workgroup per stream.  linear.0 (9 -> H) + ReLU + linear.2 (gLN over F x T x H, weight per f) + linear.3 (H -> 6)
//              + the beamformer sum_m w_m X_m.  The [F][T][H] activation is never stored: pass 1 takes sum and sum of squares (per
//              bin in fp32, per thread in double, one fixed tree across the workgroup), pass 2 recomputes the 9 -> H layer.  The
//              weights are read with wave-uniform indices, so they come through the scalar cache as SGPR operands.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/se_engine.h"

namespace se {
int train_fail(int code, const char *fmt, ...);  // se_train.hip (owns se_train_last_error)
}

namespace {

constexpr float kEps = 1e-8f;         // GeneralBeamformer.py:11
constexpr int kPsdThreads = 256, kSeqThreads = 256, kBfThreads = 512;
constexpr int kM = 3, kRow = 16;      // microphones (the head's 9 = M*M inputs and 6 = 2M outputs are fixed); GRU input row width

template <int NT>
__device__ double block_sum(double v, double *red) {  // fixed-order tree: the same association for every launch
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float gln_scale(double var) { return 1.0f / (sqrtf((float)var + kEps) + kEps); }

struct PsdArgs {
    const float *xl;     // [S][4M*9][T][F]: last decoder output after ReLU + gLN; channel ((s*2 + ri)*M + m)*9 + k
    const float *spec;   // [S][M][T][F][2]
    const float *w[2], *b[2];   // ln_S / ln_N affine [F*T]
    float *rows[2];      // [B][F][Nc][T][16], Nc = S / B (stream-major GRU rows)
    int S, B, T, F;
};

// GRU row of segment stream s = n B + b, frequency f, frame t: stream-major [B][F][Nc][T], so that a pass of Nc segments is one
// [B F][Nc T] sequence per (utterance, frequency) - se_train_gru_pseq_fwd's ldN = 0 addressing for any number of streams
__device__ __forceinline__ long gru_row(int s, int f, int t, int B, int F, int T, int Nc) {
    const int n = s / B, b = s - n * B;
    return (((long)b * F + f) * Nc + n) * T + t;
}

__global__ __launch_bounds__(kPsdThreads) void k_gbf_psd(PsdArgs a) {
    __shared__ double red[kPsdThreads];
    const int s = blockIdx.x, T = a.T, F = a.F, FT = F * T, Nc = a.S / a.B;
    const long plane = (long)T * F;
    const float *xl = a.xl + (long)s * 4 * kM * 9 * plane;
    const float *sp = a.spec + (long)s * kM * plane * 2;
    double sum[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {
        const int t = i / F, f = i - t * F;
        // taps of the unfold: component r of bin (f, t) reads row f + kf - 1, column 2t + r + kc - 1 of the interleaved [F][2T] plane
        float ur[kM][9], ui[kM][9];
#pragma unroll
        for (int m = 0; m < kM; m++)
#pragma unroll
            for (int kf = 0; kf < 3; kf++)
#pragma unroll
                for (int kc = 0; kc < 3; kc++) {
                    const int row = f + kf - 1;
                    float v[2];
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        const int col = 2 * t + r + kc - 1;
                        v[r] = (row >= 0 && row < F && col >= 0 && col < 2 * T) ? sp[(((long)m * T + (col >> 1)) * F + row) * 2 + (col & 1)] : 0.f;
                    }
                    ur[m][3 * kf + kc] = v[0];
                    ui[m][3 * kf + kc] = v[1];
                }
        const long off = (long)t * F + f;
#pragma unroll
        for (int q = 0; q < 2; q++) {  // q = 0: speech filter S, 1: noise filter N
            float sr[kM], si[kM];
#pragma unroll
            for (int m = 0; m < kM; m++) {
                float accr = 0.f, acci = 0.f;
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    const float fr = xl[(long)(((q * 2 + 0) * kM + m) * 9 + k) * plane + off];
                    const float fi = xl[(long)(((q * 2 + 1) * kM + m) * 9 + k) * plane + off];
                    accr += fr * ur[m][k] - fi * ui[m][k];
                    acci += fr * ui[m][k] + fi * ur[m][k];
                }
                sr[m] = accr; si[m] = acci;
            }
            float phi[9];
            float ps = 0.f;
#pragma unroll
            for (int p = 0; p < kM; p++)
#pragma unroll
                for (int r = 0; r < kM; r++) {
                    phi[p * kM + r] = sr[p] * sr[r] + si[p] * si[r];
                    ps += phi[p * kM + r];
                }
            sum[q] += ps;
            float4 *o = reinterpret_cast<float4 *>(a.rows[q] + gru_row(s, f, t, a.B, F, T, Nc) * kRow);
            o[0] = make_float4(phi[0], phi[1], phi[2], phi[3]);
            o[1] = make_float4(phi[4], phi[5], phi[6], phi[7]);
            o[2] = make_float4(phi[8], 0.f, 0.f, 0.f);
            o[3] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const double n = 9.0 * FT;
    double mean[2], ss[2] = {0.0, 0.0};
    for (int q = 0; q < 2; q++) mean[q] = block_sum<kPsdThreads>(sum[q], red) / n;
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {  // rows written by this thread above, in the same order
        const int t = i / F, f = i - t * F;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const float *o = a.rows[q] + gru_row(s, f, t, a.B, F, T, Nc) * kRow;
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const float e = o[j] - (float)mean[q];
                d += (double)(e * e);
            }
            ss[q] += d;
        }
    }
    float rs[2], mu[2];
    for (int q = 0; q < 2; q++) {
        rs[q] = gln_scale(block_sum<kPsdThreads>(ss[q], red) / n);
        mu[q] = (float)mean[q];
    }
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {
        const int t = i / F, f = i - t * F;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float *o = a.rows[q] + gru_row(s, f, t, a.B, F, T, Nc) * kRow;
            const float w = a.w[q][f * T + t], b = a.b[q][f * T + t];
#pragma unroll
            for (int j = 0; j < 9; j++) o[j] = (o[j] - mu[q]) * rs[q] * w + b;
        }
    }
}

struct SeqArgs {
    const float *h[2];     // last-layer GRU outputs of gru_S / gru_N, rows [B][F][Nc][T] of H
    const float *fw[2], *fb[2];   // fc_output_layer [9][H], [9]
    const float *nw[2], *nb[2];   // SequenceModel.norm [9], [9]
    float *phi;            // [S][F][T][9] = Phi_S * Phi_N
    float *y[2];           // optional: the two SequenceModel outputs [S][F][T][9]
    int S, B, F, T, H;
};

constexpr int kSeqMaxT = 64;

__global__ __launch_bounds__(kSeqThreads) void k_gbf_seq(SeqArgs a) {
    __shared__ float v[2][kSeqMaxT][9];
    __shared__ float stat[2][2];
    const int sf = blockIdx.x, T = a.T, H = a.H, s = sf / a.F, f = sf - s * a.F;
    const long r0 = gru_row(s, f, 0, a.B, a.F, T, a.S / a.B);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = kSeqThreads / 64;
    for (int p = wave; p < 2 * T; p += NW) {  // (model, step) pairs, one per wave
        const int q = p / T, t = p - q * T;
        const float *h = a.h[q] + (r0 + t) * H;
        const float *fw = a.fw[q];
        float part[9];
#pragma unroll
        for (int j = 0; j < 9; j++) part[j] = 0.f;
        for (int k = lane; k < H; k += 64) {
            const float hk = h[k];
#pragma unroll
            for (int j = 0; j < 9; j++) part[j] += hk * fw[j * H + k];
        }
#pragma unroll
        for (int j = 0; j < 9; j++) {
            float x = part[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
            part[j] = x;
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; j++) v[q][t][j] = fmaxf(part[j] + a.fb[q][j], 0.f);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {  // gLN over the T x 9 values of this sequence, two passes in double (189 values: one thread)
        const int q = threadIdx.x;
        double s = 0.0;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 9; j++) s += v[q][t][j];
        const double mean = s / (9.0 * T);
        double ss = 0.0;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 9; j++) {
                const float e = v[q][t][j] - (float)mean;
                ss += (double)(e * e);
            }
        stat[q][0] = (float)mean;
        stat[q][1] = gln_scale(ss / (9.0 * T));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * T; i += kSeqThreads) {
        const int t = i / 9, j = i - t * 9;
        float y[2];
#pragma unroll
        for (int q = 0; q < 2; q++) y[q] = (v[q][t][j] - stat[q][0]) * stat[q][1] * a.nw[q][j] + a.nb[q][j];
        const long o = ((long)sf * T + t) * 9 + j;
        a.phi[o] = y[0] * y[1];
        if (a.y[0]) a.y[0][o] = y[0];
        if (a.y[1]) a.y[1][o] = y[1];
    }
}

struct BfArgs {
    const float *phi;    // [S][F][T][9]
    const float *spec;   // [S][M][T][F][2]
    const float *w0, *b0;   // linear.0 [H][9], [H]
    const float *g, *beta;  // linear.2 [F], [F]
    const float *w3, *b3;   // linear.3 [6][H], [6]
    float *Y;            // [S][T][F][2]
    float *wout;         // optional: the beamforming weights [S][F][T][6]
    int S, T, F, H;
};

__global__ __launch_bounds__(kBfThreads) void k_gbf_bf(BfArgs a) {
    __shared__ double red[kBfThreads];
    const int s = blockIdx.x, T = a.T, F = a.F, H = a.H, FT = F * T;
    const float *phi_s = a.phi + (long)s * FT * 9;
    double sum = 0.0, sumsq = 0.0;
    for (int i = threadIdx.x; i < FT; i += kBfThreads) {
        const int t = i / F, f = i - t * F;
        float x[9];
        const float *p = phi_s + ((long)f * T + t) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) x[j] = p[j];
        float ps = 0.f, pss = 0.f;
        for (int h = 0; h < H; h++) {
            float z = a.b0[h];
#pragma unroll
            for (int j = 0; j < 9; j++) z += a.w0[h * 9 + j] * x[j];
            z = fmaxf(z, 0.f);
            ps += z;
            pss += z * z;
        }
        sum += ps;
        sumsq += pss;
    }
    const double n = (double)FT * H;
    const double mean = block_sum<kBfThreads>(sum, red) / n;
    const double var = fmax(block_sum<kBfThreads>(sumsq, red) / n - mean * mean, 0.0);
    const float mu = (float)mean, rs = gln_scale(var);
    for (int i = threadIdx.x; i < FT; i += kBfThreads) {
        const int t = i / F, f = i - t * F;
        float x[9];
        const float *p = phi_s + ((long)f * T + t) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) x[j] = p[j];
        const float gs = rs * a.g[f], be = a.beta[f];
        float w[6];
#pragma unroll
        for (int o = 0; o < 6; o++) w[o] = a.b3[o];
        for (int h = 0; h < H; h++) {
            float z = a.b0[h];
#pragma unroll
            for (int j = 0; j < 9; j++) z += a.w0[h * 9 + j] * x[j];
            z = (fmaxf(z, 0.f) - mu) * gs + be;
#pragma unroll
            for (int o = 0; o < 6; o++) w[o] += a.w3[o * H + h] * z;
        }
        // Y = sum_m w_m X_m, plain complex product (the reference's .conj() acts on a real tensor: a no-op)
        float yr = 0.f, yi = 0.f;
#pragma unroll
        for (int m = 0; m < kM; m++) {
            const float *X = a.spec + ((((long)s * kM + m) * T + t) * F + f) * 2;
            const float xr = X[0], xi = X[1];
            yr += w[2 * m] * xr - w[2 * m + 1] * xi;
            yi += w[2 * m] * xi + w[2 * m + 1] * xr;
        }
        float *y = a.Y + (((long)s * T + t) * F + f) * 2;
        y[0] = yr;
        y[1] = yi;
        if (a.wout) {
            float *wo = a.wout + (((long)s * F + f) * T + t) * 6;
#pragma unroll
            for (int o = 0; o < 6; o++) wo[o] = w[o];
        }
    }
}

int launched(const char *what) {
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "%s launch failed", what);
}

}  // namespace

extern "C" {

int se_gbf_psd_fwd(const float *xl, const float *spec, const float *wS, const float *bS, const float *wN, const float *bN, float *rowsS, float *rowsN,
                   int S, int B, int M, int T, int F, void *stream) {
    if (B <= 0 || S % B) return se::train_fail(SE_ERR_ARG, "se_gbf_psd_fwd: %d streams are not whole segments of %d utterances", S, B);
    if (!xl || !spec || !wS || !bS || !wN || !bN || !rowsS || !rowsN || S <= 0 || T <= 0 || F <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_psd_fwd: null / bad argument");
    if (M != kM) return se::train_fail(SE_ERR_ARG, "se_gbf_psd_fwd: %d microphones; the beamforming head is built for 3 (linear 9 -> H -> 6)", M);
    PsdArgs a{xl, spec, {wS, wN}, {bS, bN}, {rowsS, rowsN}, S, B, T, F};
    hipLaunchKernelGGL(k_gbf_psd, dim3(S), dim3(kPsdThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_psd_fwd");
}

int se_gbf_seq_fwd(const float *hS, const float *hN, const float *fcS_w, const float *fcS_b, const float *nS_w, const float *nS_b, const float *fcN_w,
                   const float *fcN_b, const float *nN_w, const float *nN_b, float *phi, float *yS, float *yN, int S, int B, int F, int T, int H, void *stream) {
    if (B <= 0 || S % B) return se::train_fail(SE_ERR_ARG, "se_gbf_seq_fwd: %d streams are not whole segments of %d utterances", S, B);
    if (!hS || !hN || !fcS_w || !fcS_b || !nS_w || !nS_b || !fcN_w || !fcN_b || !nN_w || !nN_b || !phi || S <= 0 || F <= 0 || H <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_seq_fwd: null / bad argument");
    if (T <= 0 || T > kSeqMaxT) return se::train_fail(SE_ERR_ARG, "se_gbf_seq_fwd: %d frames per segment (at most %d)", T, kSeqMaxT);
    SeqArgs a{{hS, hN}, {fcS_w, fcN_w}, {fcS_b, fcN_b}, {nS_w, nN_w}, {nS_b, nN_b}, phi, {yS, yN}, S, B, F, T, H};
    hipLaunchKernelGGL(k_gbf_seq, dim3((unsigned)((long)S * F)), dim3(kSeqThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_seq_fwd");
}

int se_gbf_bf_fwd(const float *phi, const float *spec, const float *w0, const float *b0, const float *g, const float *beta, const float *w3,
                  const float *b3, float *Y, float *wout, int S, int M, int T, int F, int H, void *stream) {
    if (!phi || !spec || !w0 || !b0 || !g || !beta || !w3 || !b3 || !Y || S <= 0 || T <= 0 || F <= 0 || H <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_bf_fwd: null / bad argument");
    if (M != kM) return se::train_fail(SE_ERR_ARG, "se_gbf_bf_fwd: %d microphones; the beamforming head is built for 3 (linear 9 -> H -> 6)", M);
    BfArgs a{phi, spec, w0, b0, g, beta, w3, b3, Y, wout, S, T, F, H};
    hipLaunchKernelGGL(k_gbf_bf, dim3(S), dim3(kBfThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_bf_fwd");
}

}  // extern "C"
