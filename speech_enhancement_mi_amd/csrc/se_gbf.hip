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
//
// Backward (training, general_beamformer.GBFFunction): the same three stages in reverse, one workgroup per stream / sequence again.
// Every forward statistic is recomputed from the saved inputs rather than stored.  Parameter gradients leave as per-stream slabs or
// as materialised [rows][n] planes which the caller folds with se_train_colsum_tall / se_train_gemm_tn_det: no atomics, fixed order.
//   k_gbf_bf_bwd   irfft weights on dY, dw = dY conj-free product with X, linear.3, gLN_F, ReLU, linear.0 -> dphi
//   k_gbf_seq_bwd  dPhi -> dyS / dyN, SequenceModel.norm, ReLU, fc_output_layer -> d(last-layer GRU output rows)
//   k_gbf_psd_bwd  d(GRU input rows) -> ln_S / ln_N, Phi = sr sr^T + si si^T, the complex 3x3 filter -> dxl
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

// ---- backward -------------------------------------------------------------------------------------------------------------------
// gLN backward for y = (x - mean) * r, r = 1 / (sigma + eps), sigma = sqrt(var + eps):
//   dx = r (dy - mean(dy) - y mean(dy y) (sigma + eps) / sigma)
__device__ __forceinline__ float gln_kf(double var) {
    const float sg = sqrtf((float)var + kEps);
    return (sg + kEps) / sg;
}

struct BfBwdArgs {
    const float *dY;     // [S][T][F][2]: raw se_sig_stft of the segment gradient
    const float *phi, *spec;
    const float *w0, *b0, *g, *beta, *w3;
    float *dphi;         // [S][F][T][9]
    float *dpre;         // [S*F*T][H]: gradient at linear.0's output (rows s*F*T + f*T + t)
    float *act;          // [S*F*T][H]: linear.3's input (the gLN output)
    float *dw;           // [S*F*T][8]: gradient of the beamforming weights, columns 6, 7 zero
    float *pg, *pb;      // [S][T][F]: per-bin partial sums for linear.2's weight / bias
    int S, T, F, H;
    float inv_nfft;
};

__device__ __forceinline__ void bf_dw(const BfBwdArgs &a, int s, int t, int f, float dw[6]) {
    const int T = a.T, F = a.F;
    const float sc = (f == 0 || f == F - 1) ? a.inv_nfft : 2.0f * a.inv_nfft;   // irfft adjoint (k_tmask_bwd)
    const float *d = a.dY + (((long)s * T + t) * F + f) * 2;
    const float gr = d[0] * sc, gi = (f == 0 || f == F - 1) ? 0.0f : d[1] * sc;  // C2R ignores Im of DC / Nyquist
#pragma unroll
    for (int m = 0; m < kM; m++) {
        const float *X = a.spec + ((((long)s * kM + m) * T + t) * F + f) * 2;
        const float xr = X[0], xi = X[1];
        dw[2 * m] = gr * xr + gi * xi;
        dw[2 * m + 1] = -gr * xi + gi * xr;
    }
}

__global__ __launch_bounds__(kBfThreads) void k_gbf_bf_bwd(BfBwdArgs a) {
    __shared__ double red[kBfThreads];
    const int s = blockIdx.x, T = a.T, F = a.F, H = a.H, FT = F * T;
    const float *phi_s = a.phi + (long)s * FT * 9;
    double sum = 0.0, sumsq = 0.0;
    for (int i = threadIdx.x; i < FT; i += kBfThreads) {  // statistics exactly as k_gbf_bf
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
    const float mu = (float)mean, rs = gln_scale(var), kf = gln_kf(var);
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < FT; i += kBfThreads) {  // dw, linear.3, gLN affine; sums of dzn and dzn * zn
        const int t = i / F, f = i - t * F;
        const long row = (long)s * FT + (long)f * T + t;
        float x[9], dw[6];
        const float *p = phi_s + ((long)f * T + t) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) x[j] = p[j];
        bf_dw(a, s, t, f, dw);
        const float gf = a.g[f], be = a.beta[f];
        float ps1 = 0.f, ps2 = 0.f, pg = 0.f, pb = 0.f;
        float *act = a.act + row * H;
        for (int h = 0; h < H; h++) {
            float z = a.b0[h];
#pragma unroll
            for (int j = 0; j < 9; j++) z += a.w0[h * 9 + j] * x[j];
            const float zn = (fmaxf(z, 0.f) - mu) * rs;
            act[h] = zn * gf + be;
            float da = 0.f;
#pragma unroll
            for (int o = 0; o < 6; o++) da += a.w3[o * H + h] * dw[o];
            const float dzn = da * gf;
            ps1 += dzn;
            ps2 += dzn * zn;
            pg += da * zn;
            pb += da;
        }
        s1 += ps1;
        s2 += ps2;
        float4 *wo = reinterpret_cast<float4 *>(a.dw + row * 8);
        wo[0] = make_float4(dw[0], dw[1], dw[2], dw[3]);
        wo[1] = make_float4(dw[4], dw[5], 0.f, 0.f);
        a.pg[((long)s * T + t) * F + f] = pg;
        a.pb[((long)s * T + t) * F + f] = pb;
    }
    const float m1 = (float)(block_sum<kBfThreads>(s1, red) / n), m2 = (float)(block_sum<kBfThreads>(s2, red) / n) * kf;
    for (int i = threadIdx.x; i < FT; i += kBfThreads) {  // back through gLN, ReLU, linear.0
        const int t = i / F, f = i - t * F;
        const long row = (long)s * FT + (long)f * T + t;
        float x[9], dw[6], dx[9];
        const float *p = phi_s + ((long)f * T + t) * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            x[j] = p[j];
            dx[j] = 0.f;
        }
        bf_dw(a, s, t, f, dw);
        const float gf = a.g[f];
        float *dpre = a.dpre + row * H;
        for (int h = 0; h < H; h++) {
            float z = a.b0[h];
#pragma unroll
            for (int j = 0; j < 9; j++) z += a.w0[h * 9 + j] * x[j];
            const float zn = (fmaxf(z, 0.f) - mu) * rs;
            float da = 0.f;
#pragma unroll
            for (int o = 0; o < 6; o++) da += a.w3[o * H + h] * dw[o];
            const float dz = z > 0.f ? rs * (da * gf - m1 - zn * m2) : 0.f;
            dpre[h] = dz;
#pragma unroll
            for (int j = 0; j < 9; j++) dx[j] += a.w0[h * 9 + j] * dz;
        }
        float *o = a.dphi + row * 9;
#pragma unroll
        for (int j = 0; j < 9; j++) o[j] = dx[j];
    }
}

struct SeqBwdArgs {
    const float *dphi;          // [S][F][T][9]
    const float *h[2];          // last-layer GRU outputs, rows [B][F][Nc][T] of H
    const float *fw[2], *fb[2], *nw[2], *nb[2];
    float *dh[2];               // gradient of the last-layer GRU outputs, same rows
    float *dv[2];               // [rows][16]: gradient at fc_output_layer's output, columns 9..15 zero
    float *part;                // [S*F][54]: per model q: norm.weight (9), norm.bias (9), fc_output_layer.bias (9) at q * 27
    int S, B, F, T, H;
};

__global__ __launch_bounds__(kSeqThreads) void k_gbf_seq_bwd(SeqBwdArgs a) {
    __shared__ float v[2][kSeqMaxT][9], yn[2][kSeqMaxT][9], dy[2][kSeqMaxT][9];
    __shared__ float stat[2][4];
    const int sf = blockIdx.x, T = a.T, H = a.H, s = sf / a.F, f = sf - s * a.F;
    const long r0 = gru_row(s, f, 0, a.B, a.F, T, a.S / a.B);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = kSeqThreads / 64;
    for (int p = wave; p < 2 * T; p += NW) {  // fc + ReLU exactly as k_gbf_seq
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
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        double sm = 0.0;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 9; j++) sm += v[q][t][j];
        const double mean = sm / (9.0 * T);
        double ss = 0.0;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 9; j++) {
                const float e = v[q][t][j] - (float)mean;
                ss += (double)(e * e);
            }
        stat[q][0] = (float)mean;
        stat[q][1] = gln_scale(ss / (9.0 * T));
        stat[q][2] = gln_kf(ss / (9.0 * T));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * T; i += kSeqThreads) {  // phi = yS * yN: each factor's gradient is dphi times the other
        const int t = i / 9, j = i - t * 9;
        float z[2], y[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            z[q] = (v[q][t][j] - stat[q][0]) * stat[q][1];
            y[q] = z[q] * a.nw[q][j] + a.nb[q][j];
        }
        const float d = a.dphi[((long)sf * T + t) * 9 + j];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            yn[q][t][j] = z[q];
            dy[q][t][j] = d * y[1 - q];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2) {  // mean(dyn) and mean(dyn * yn) per model, dyn = dy * weight
        const int q = threadIdx.x;
        double m1 = 0.0, m2 = 0.0;
        for (int t = 0; t < T; t++)
            for (int j = 0; j < 9; j++) {
                const float dn = dy[q][t][j] * a.nw[q][j];
                m1 += dn;
                m2 += (double)(dn * yn[q][t][j]);
            }
        stat[q][3] = (float)(m1 / (9.0 * T));
        stat[q][2] *= (float)(m2 / (9.0 * T));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * 9 * T; i += kSeqThreads) {  // gLN, ReLU -> the fc output gradient (in place of v)
        const int q = i / (9 * T), r = i - q * 9 * T, t = r / 9, j = r - t * 9;
        const float dn = dy[q][t][j] * a.nw[q][j];
        const float d = v[q][t][j] > 0.f ? stat[q][1] * (dn - stat[q][3] - yn[q][t][j] * stat[q][2]) : 0.f;
        v[q][t][j] = d;
    }
    __syncthreads();
    if (threadIdx.x < 18) {  // per-sequence parameter slabs, summed over t in order
        const int q = threadIdx.x / 9, j = threadIdx.x - q * 9;
        float gw = 0.f, gb = 0.f, gfb = 0.f;
        for (int t = 0; t < T; t++) {
            gw += dy[q][t][j] * yn[q][t][j];
            gb += dy[q][t][j];
            gfb += v[q][t][j];
        }
        float *o = a.part + (long)sf * 54 + q * 27;
        o[j] = gw;
        o[9 + j] = gb;
        o[18 + j] = gfb;
    }
    for (int i = threadIdx.x; i < 2 * T * 16; i += kSeqThreads) {
        const int q = i / (T * 16), r = i - q * T * 16, t = r / 16, j = r - t * 16;
        a.dv[q][(r0 + t) * 16 + j] = j < 9 ? v[q][t][j] : 0.f;
    }
    for (int i = threadIdx.x; i < 2 * T * H; i += kSeqThreads) {  // d h = fc^T d v
        const int q = i / (T * H), r = i - q * T * H, t = r / H, k = r - t * H;
        const float *fw = a.fw[q];
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 9; j++) acc += fw[j * H + k] * v[q][t][j];
        a.dh[q][(r0 + t) * H + k] = acc;
    }
}

struct PsdBwdArgs {
    const float *xl, *spec;
    const float *w[2], *b[2];   // ln_S / ln_N affine [F*T]
    const float *drows[2];      // [B][F][Nc][T][16]: gradient of the GRU input rows (columns 0..8)
    float *dxl;                 // [S][4M*9][T][F]
    float *part;                // [S][4][F*T]: ln_S weight, ln_S bias, ln_N weight, ln_N bias
    int S, B, T, F;
};

// the unfold taps and the two filtered microphone vectors of bin (f, t), as k_gbf_psd
__device__ __forceinline__ void psd_bin(const PsdBwdArgs &a, int s, int f, int t, float ur[kM][9], float ui[kM][9], float sr[2][kM],
                                        float si[2][kM]) {
    const int T = a.T, F = a.F;
    const long plane = (long)T * F;
    const float *xl = a.xl + (long)s * 4 * kM * 9 * plane;
    const float *sp = a.spec + (long)s * kM * plane * 2;
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
    for (int q = 0; q < 2; q++)
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
            sr[q][m] = accr;
            si[q][m] = acci;
        }
}

__device__ __forceinline__ void psd_phi(const float sr[kM], const float si[kM], float phi[9]) {
#pragma unroll
    for (int p = 0; p < kM; p++)
#pragma unroll
        for (int r = 0; r < kM; r++) phi[p * kM + r] = sr[p] * sr[r] + si[p] * si[r];
}

__global__ __launch_bounds__(kPsdThreads) void k_gbf_psd_bwd(PsdBwdArgs a) {
    __shared__ double red[kPsdThreads];
    const int s = blockIdx.x, T = a.T, F = a.F, FT = F * T, Nc = a.S / a.B;
    float ur[kM][9], ui[kM][9], sr[2][kM], si[2][kM];
    double sum[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {  // statistics as k_gbf_psd
        const int t = i / F, f = i - t * F;
        psd_bin(a, s, f, t, ur, ui, sr, si);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float phi[9];
            psd_phi(sr[q], si[q], phi);
            float ps = 0.f;
#pragma unroll
            for (int j = 0; j < 9; j++) ps += phi[j];
            sum[q] += ps;
        }
    }
    const double n = 9.0 * FT;
    double mean[2], ss[2] = {0.0, 0.0};
    for (int q = 0; q < 2; q++) mean[q] = block_sum<kPsdThreads>(sum[q], red) / n;
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {
        const int t = i / F, f = i - t * F;
        psd_bin(a, s, f, t, ur, ui, sr, si);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float phi[9];
            psd_phi(sr[q], si[q], phi);
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const float e = phi[j] - (float)mean[q];
                d += (double)(e * e);
            }
            ss[q] += d;
        }
    }
    float rs[2], mu[2], kf[2];
    for (int q = 0; q < 2; q++) {
        const double var = block_sum<kPsdThreads>(ss[q], red) / n;
        rs[q] = gln_scale(var);
        kf[q] = gln_kf(var);
        mu[q] = (float)mean[q];
    }
    double g1[2] = {0.0, 0.0}, g2[2] = {0.0, 0.0};
    float *part = a.part + (long)s * 4 * FT;
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {  // affine gradients per bin; sums of dyn and dyn * yn
        const int t = i / F, f = i - t * F;
        const int bin = f * T + t;
        psd_bin(a, s, f, t, ur, ui, sr, si);
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float phi[9];
            psd_phi(sr[q], si[q], phi);
            const float *d = a.drows[q] + gru_row(s, f, t, a.B, F, T, Nc) * kRow;
            const float w = a.w[q][bin];
            float pw = 0.f, pb = 0.f, p1 = 0.f, p2 = 0.f;
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const float yn = (phi[j] - mu[q]) * rs[q];
                pw += d[j] * yn;
                pb += d[j];
                p1 += d[j] * w;
                p2 += d[j] * w * yn;
            }
            part[(2 * q) * FT + bin] = pw;
            part[(2 * q + 1) * FT + bin] = pb;
            g1[q] += p1;
            g2[q] += p2;
        }
    }
    float m1[2], m2[2];
    for (int q = 0; q < 2; q++) {
        m1[q] = (float)(block_sum<kPsdThreads>(g1[q], red) / n);
        m2[q] = (float)(block_sum<kPsdThreads>(g2[q], red) / n) * kf[q];
    }
    const long plane = (long)T * F;
    float *dxl = a.dxl + (long)s * 4 * kM * 9 * plane;
    for (int i = threadIdx.x; i < FT; i += kPsdThreads) {  // dPhi -> dsr, dsi -> the filter taps
        const int t = i / F, f = i - t * F;
        const int bin = f * T + t;
        psd_bin(a, s, f, t, ur, ui, sr, si);
        const long off = (long)t * F + f;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            float phi[9], dp[9];
            psd_phi(sr[q], si[q], phi);
            const float *d = a.drows[q] + gru_row(s, f, t, a.B, F, T, Nc) * kRow;
            const float w = a.w[q][bin];
#pragma unroll
            for (int j = 0; j < 9; j++) {
                const float yn = (phi[j] - mu[q]) * rs[q];
                dp[j] = rs[q] * (d[j] * w - m1[q] - yn * m2[q]);
            }
            float dsr[kM], dsi[kM];
#pragma unroll
            for (int p = 0; p < kM; p++) {
                float ar = 0.f, ai = 0.f;
#pragma unroll
                for (int r = 0; r < kM; r++) {
                    const float e = dp[p * kM + r] + dp[r * kM + p];
                    ar += e * sr[q][r];
                    ai += e * si[q][r];
                }
                dsr[p] = ar;
                dsi[p] = ai;
            }
#pragma unroll
            for (int m = 0; m < kM; m++)
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    dxl[(long)(((q * 2 + 0) * kM + m) * 9 + k) * plane + off] = dsr[m] * ur[m][k] + dsi[m] * ui[m][k];
                    dxl[(long)(((q * 2 + 1) * kM + m) * 9 + k) * plane + off] = -dsr[m] * ui[m][k] + dsi[m] * ur[m][k];
                }
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

int se_gbf_bf_bwd(const float *dY, const float *phi, const float *spec, const float *w0, const float *b0, const float *g, const float *beta,
                  const float *w3, float *dphi, float *dpre, float *act, float *dw, float *pg, float *pb, int S, int M, int T, int F, int H,
                  int n_fft, void *stream) {
    if (!dY || !phi || !spec || !w0 || !b0 || !g || !beta || !w3 || !dphi || !dpre || !act || !dw || !pg || !pb || S <= 0 || T <= 0 || F <= 0 ||
        H <= 0 || n_fft <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_bf_bwd: null / bad argument");
    if (M != kM) return se::train_fail(SE_ERR_ARG, "se_gbf_bf_bwd: %d microphones; the beamforming head is built for 3 (linear 9 -> H -> 6)", M);
    BfBwdArgs a{dY, phi, spec, w0, b0, g, beta, w3, dphi, dpre, act, dw, pg, pb, S, T, F, H, 1.0f / (float)n_fft};
    hipLaunchKernelGGL(k_gbf_bf_bwd, dim3(S), dim3(kBfThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_bf_bwd");
}

int se_gbf_seq_bwd(const float *dphi, const float *hS, const float *hN, const float *fcS_w, const float *fcS_b, const float *nS_w,
                   const float *nS_b, const float *fcN_w, const float *fcN_b, const float *nN_w, const float *nN_b, float *dhS, float *dhN,
                   float *dvS, float *dvN, float *part, int S, int B, int F, int T, int H, void *stream) {
    if (B <= 0 || S % B) return se::train_fail(SE_ERR_ARG, "se_gbf_seq_bwd: %d streams are not whole segments of %d utterances", S, B);
    if (!dphi || !hS || !hN || !fcS_w || !fcS_b || !nS_w || !nS_b || !fcN_w || !fcN_b || !nN_w || !nN_b || !dhS || !dhN || !dvS || !dvN || !part ||
        S <= 0 || F <= 0 || H <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_seq_bwd: null / bad argument");
    if (T <= 0 || T > kSeqMaxT) return se::train_fail(SE_ERR_ARG, "se_gbf_seq_bwd: %d frames per segment (at most %d)", T, kSeqMaxT);
    SeqBwdArgs a{dphi, {hS, hN}, {fcS_w, fcN_w}, {fcS_b, fcN_b}, {nS_w, nN_w}, {nS_b, nN_b}, {dhS, dhN}, {dvS, dvN}, part, S, B, F, T, H};
    hipLaunchKernelGGL(k_gbf_seq_bwd, dim3((unsigned)((long)S * F)), dim3(kSeqThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_seq_bwd");
}

int se_gbf_psd_bwd(const float *xl, const float *spec, const float *wS, const float *bS, const float *wN, const float *bN, const float *drowsS,
                   const float *drowsN, float *dxl, float *part, int S, int B, int M, int T, int F, void *stream) {
    if (B <= 0 || S % B) return se::train_fail(SE_ERR_ARG, "se_gbf_psd_bwd: %d streams are not whole segments of %d utterances", S, B);
    if (!xl || !spec || !wS || !bS || !wN || !bN || !drowsS || !drowsN || !dxl || !part || S <= 0 || T <= 0 || F <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gbf_psd_bwd: null / bad argument");
    if (M != kM) return se::train_fail(SE_ERR_ARG, "se_gbf_psd_bwd: %d microphones; the beamforming head is built for 3 (linear 9 -> H -> 6)", M);
    PsdBwdArgs a{xl, spec, {wS, wN}, {bS, bN}, {drowsS, drowsN}, dxl, part, S, B, T, F};
    hipLaunchKernelGGL(k_gbf_psd_bwd, dim3(S), dim3(kPsdThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gbf_psd_bwd");
}

}  // extern "C"
