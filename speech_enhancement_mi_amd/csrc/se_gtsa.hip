// se_gtsa.hip - the GTSA transformer (reference GTSA.py:139-307) behind se_gtsa_* (include/se_engine.h).
//
// Layout: S = Nc windows x B utterances, window-major (s = n B + b), ONE activation layout x [S][C][T][Fs] for both layer kinds, C = 2M - 1 = 5
// features, Fs >= F the row stride (F rounded up to the GEMM's K % 8, the pad columns kept zero by every kernel that writes x).  Even
// layers see rows (s, c, t) contiguous in F (their nn.Linear layers are se_train_gemm calls on those rows); odd-layer kernels index rows
// (s, f, t) with the five features at stride T * Fs.  No transposes go through memory.
//
// The rolling key / value buffer is a TAPE per (sequence, head): rows [0, maxlen) are the carried buffer, rows maxlen + n T + t the
// keys / values projected from window n of this call.  Window n attends to tape rows [(n + 1) T, (n + 1) T + maxlen), which is the
// reference's cat([bk[:, T:], k]) applied n + 1 times.  The tape is virtual: the carried part [(b U + u) Hh + h][maxlen][D] and the new
// part (rows of the projection output) stay where they are; se_gtsa_tape writes the last maxlen rows as the next carried part.
//
//   k_gtsa_feat     |X| of every microphone and atan2 phase differences (GTSA.py:279-284)
//   k_gtsa_attn<D>  one workgroup per (stream, sequence, head): softmax(|Q K^T G / sqrt(model_dim)|) V over the window, keys walked in
//                   tiles of 64 with a running maximum and sum; G from delta in the kernel; scores never leave the chip
//   k_gtsa_tape     the carried K / V a call leaves behind (k_gtsa_tape_rows: every stream's tape ends at its own window count)
//   k_gtsa_addnorm  y = gLN(a + x) per (s, c) sequence over T x F, affine per f (even layers: after attention and after the FFN)
//   k_gtsa_qkv5     the 5 x 5 q / k / v projections of an odd layer, written as rows [S][F][T][16] (q 0..4, k 5..9, v 10..14)
//   k_gtsa_tail5    an odd layer after attention in one launch: output projection, residual, gLN, FFN 5 -> fn -> 5 (fn walked with
//                   the 5-wide accumulator in registers, the hidden activation never stored), residual, gLN
//   k_gtsa_gather3  the k = 3 convolution's GEMM rows: three frames (t - 2, t - 1, t) of all 5 F inputs per output frame
//   k_gtsa_lastframes_rows  the two input frames last_conv carries on: the end of every stream's own last window of the pass
//   k_gtsa_out      conv_trans * sigmoid(conv_gated), gLN over 2F x T, decompress_cIRM, complex product with microphone 0
//
// fp32 arithmetic, statistics combined in double, no atomics, every reduction in a fixed order that does not depend on S: results are
// bit-reproducible and do not depend on how a call is cut into passes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/se_engine.h"

namespace se {
int train_fail(int code, const char *fmt, ...);  // se_train.hip (owns se_train_last_error)
}

namespace {

constexpr int kC = 5;          // features per bin: 2M - 1 with M = 3 microphones
constexpr int kMaxT = 32;      // frames per window (queries per workgroup; 8 rows per thread in k_gtsa_tail5)
constexpr int kMaxLen = 4096;  // -(i - j)^2 stays exact in fp32
constexpr int kKT = 64;        // keys per tile: one per lane
constexpr int kNormMax = 8192; // T * F values of one even-layer sequence held in LDS
constexpr int kThreads = 256, kWaves = kThreads / 64, kRowsPerThread = kMaxT / kWaves;

__device__ __forceinline__ float gln_scale(double var) { return 1.0f / (sqrtf((float)var + 1e-10f) + 1e-8f); }  // GTSA.py:123

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

// ---- features ----------------------------------------------------------------------------------------------------------------------
struct FeatArgs {
    const float2 *spec;  // [S][M][T][F]
    float *x;            // [S][2M-1][T][Fs]
    int M, T, F, Fs;
};

__global__ __launch_bounds__(kThreads) void k_gtsa_feat(FeatArgs a) {
    const int s = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.T * a.Fs) return;
    const int t = i / a.Fs, f = i - t * a.Fs, C = 2 * a.M - 1;
    const long cs = (long)a.T * a.Fs;
    float *o = a.x + (long)s * C * cs + (long)t * a.Fs + f;
    if (f >= a.F) {
        for (int c = 0; c < C; c++) o[c * cs] = 0.f;
        return;
    }
    const float2 *sp = a.spec + ((long)s * a.M * a.T + t) * a.F + f;
    float ang0 = 0.f;
    for (int m = 0; m < a.M; m++) {
        const float2 v = sp[(long)m * a.T * a.F];
        o[m * cs] = sqrtf(v.x * v.x + v.y * v.y + 1e-10f);
        // a bin that is exactly zero has no phase: 0 whatever the signs of its zeros (atan2(+0, -0) would be pi).  On an all-zero
        // frame every microphone is zero together, so the difference is 0 as in the reference, whose FFT gives all of them one sign.
        const float ang = (v.x == 0.f && v.y == 0.f) ? 0.f : atan2f(v.y, v.x);
        if (m == 0) ang0 = ang;
        else o[(a.M + m - 1) * cs] = ang0 - ang;
    }
}

// ---- attention over the tape -------------------------------------------------------------------------------------------------------
struct AttnArgs {
    const float *q, *kn, *vn;  // row ((s U + u) T + t) at stride ldq / ldk, head h at column h D
    const float *kc, *vc;      // carried [(b U + u) Hh + h][maxlen][D]
    float *out;                // row ((s U + u) T + t) at stride ldo, head h at column h D
    const float *delta;        // [1]
    int ldq, ldk, ldo, B, U, Hh, T, maxlen;
    float d;                   // sqrt(model_dim)
};

template <int D>
__global__ __launch_bounds__(kThreads) void k_gtsa_attn(AttnArgs a) {
    constexpr int NO = (kMaxT * D + kThreads - 1) / kThreads;
    __shared__ float sq[kMaxT][D];
    __shared__ float sk[kKT][D];
    __shared__ float sv[kKT][D];
    __shared__ float sp[kMaxT][kKT];
    __shared__ float sscale[kMaxT], ssum[kMaxT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, uh = blockIdx.y, u = uh / a.Hh, h = uh - u * a.Hh;
    const int B = a.B, U = a.U, T = a.T, maxlen = a.maxlen, n = s / B, b = s - n * B;
    const long qrow0 = ((long)s * U + u) * T;
    for (int i = tid; i < T * D; i += kThreads) {
        const int t = i / D, d = i - t * D;
        sq[t][d] = a.q[(qrow0 + t) * a.ldq + h * D + d];
    }
    float m_run[kRowsPerThread], l_run[kRowsPerThread], acc[NO];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++) { m_run[k] = 0.f; l_run[k] = 0.f; }  // scores are |.| >= 0: 0 is a lower bound of the maximum
#pragma unroll
    for (int k = 0; k < NO; k++) acc[k] = 0.f;
    const float dl = a.delta[0], den = dl * dl + 1e-8f;
    const int w0 = (n + 1) * T;  // first tape row of this window
    const long crow0 = ((long)(b * U + u) * a.Hh + h) * maxlen;
    for (int j0 = 0; j0 < maxlen; j0 += kKT) {
        __syncthreads();  // the previous tile is consumed (and sq is written, first time round)
        for (int i = tid; i < kKT * D; i += kThreads) {
            const int j = i / D, d = i - j * D, jj = j0 + j;
            float kv = 0.f, vv = 0.f;
            if (jj < maxlen) {
                const int r = w0 + jj;
                if (r < maxlen) {
                    const long off = (crow0 + r) * D + d;
                    kv = a.kc[off]; vv = a.vc[off];
                } else {
                    const int rr = r - maxlen, nn = rr / T, tt = rr - nn * T;  // nn <= n: a window never reads beyond its own keys
                    const long off = ((((long)nn * B + b) * U + u) * T + tt) * a.ldk + h * D + d;
                    kv = a.kn[off]; vv = a.vn[off];
                }
            }
            sk[j][d] = kv; sv[j][d] = vv;
        }
        __syncthreads();
        float kreg[D];
#pragma unroll
        for (int d = 0; d < D; d++) kreg[d] = sk[lane][d];
        const int jj = j0 + lane;
        const bool live = jj < maxlen;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; k++) {
            const int t = wave + kWaves * k;
            if (t < T) {  // wave-uniform
                float dot = 0.f;
#pragma unroll
                for (int d = 0; d < D; d++) dot += sq[t][d] * kreg[d];
                const float df = (float)(maxlen - T + t - jj);
                const float g = expf(-(df * df) / den);
                const float sc = live ? fabsf(dot * g / a.d) : 0.f;
                float mx = sc;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
                const float mnew = fmaxf(m_run[k], mx);
                const float p = live ? expf(sc - mnew) : 0.f;
                float ps = p;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) ps += __shfl_xor(ps, o);
                const float scale = expf(m_run[k] - mnew);
                l_run[k] = l_run[k] * scale + ps;
                m_run[k] = mnew;
                sp[t][lane] = p;
                if (lane == 0) sscale[t] = scale;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NO; k++) {
            const int o = tid + kThreads * k;
            if (o < T * D) {
                const int t = o / D, d = o - t * D;
                float v = acc[k] * sscale[t];
                for (int j = 0; j < kKT; j++) v += sp[t][j] * sv[j][d];
                acc[k] = v;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++) {
        const int t = wave + kWaves * k;
        if (t < T && lane == 0) ssum[t] = l_run[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NO; k++) {
        const int o = tid + kThreads * k;
        if (o < T * D) {
            const int t = o / D, d = o - t * D;
            a.out[(qrow0 + t) * a.ldo + h * D + d] = acc[k] / ssum[t];
        }
    }
}

struct TapeArgs {
    const float *kn, *vn, *kc, *vc;
    float *ko, *vo;  // [(b U + u) Hh + h][maxlen][D], not the carried input
    int ldk, Nc, B, U, Hh, D, T, maxlen;
    long total;      // B U Hh maxlen D
};

__global__ __launch_bounds__(kThreads) void k_gtsa_tape(TapeArgs a) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.total) return;
    const int d = (int)(i % a.D);
    const long row = i / a.D;
    const int r = (int)(row % a.maxlen);
    const long buh = row / a.maxlen;
    const int h = (int)(buh % a.Hh);
    const long bu = buh / a.Hh;  // b U + u
    const int tr = a.Nc * a.T + r;  // tape row
    if (tr < a.maxlen) {
        const long off = (buh * a.maxlen + tr) * a.D + d;
        a.ko[i] = a.kc[off]; a.vo[i] = a.vc[off];
    } else {
        const int rr = tr - a.maxlen, nn = rr / a.T, tt = rr - nn * a.T;  // nn < Nc
        const long b = bu / a.U, u = bu - b * a.U;
        const long off = ((((long)nn * a.B + b) * a.U + u) * a.T + tt) * a.ldk + h * a.D + d;
        a.ko[i] = a.kn[off]; a.vo[i] = a.vn[off];
    }
}

// chunk chains: stream b has cnt[b] <= Nc windows of its own in this pass, so its tape ends after cnt[b] windows.  Per element the copy
// of k_gtsa_tape with Nc replaced by the stream's own count; cnt[b] = 0 copies the carried part.
struct TapeRowsArgs {
    TapeArgs t;
    const long *cnt;  // [B], clamped to [0, Nc] here
};

__global__ __launch_bounds__(kThreads) void k_gtsa_tape_rows(TapeRowsArgs ar) {
    const TapeArgs &a = ar.t;
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.total) return;
    const int d = (int)(i % a.D);
    const long row = i / a.D;
    const int r = (int)(row % a.maxlen);
    const long buh = row / a.maxlen;
    const int h = (int)(buh % a.Hh);
    const long bu = buh / a.Hh;  // b U + u
    const long b = bu / a.U, u = bu - b * a.U;
    const long c = ar.cnt[b];
    const int own = c < 0 ? 0 : (c > a.Nc ? a.Nc : (int)c);
    const int tr = own * a.T + r;  // tape row
    if (tr < a.maxlen) {
        const long off = (buh * a.maxlen + tr) * a.D + d;
        a.ko[i] = a.kc[off]; a.vo[i] = a.vc[off];
    } else {
        const int rr = tr - a.maxlen, nn = rr / a.T, tt = rr - nn * a.T;  // nn < own
        const long off = ((((long)nn * a.B + b) * a.U + u) * a.T + tt) * a.ldk + h * a.D + d;
        a.ko[i] = a.kn[off]; a.vo[i] = a.vn[off];
    }
}

// ---- even layers: residual + gLN per (s, c) sequence ---------------------------------------------------------------------------------
struct NormArgs {
    const float *a;  // rows [nseq T] at stride lda
    const float *x;  // rows at stride Fs
    float *y;        // rows at stride Fs (may be x)
    const float *w, *b;  // [F]
    int lda, T, F, Fs;
};

__global__ __launch_bounds__(kThreads) void k_gtsa_addnorm(NormArgs a) {
    __shared__ float buf[kNormMax];
    __shared__ double red[kThreads];
    const int T = a.T, F = a.F, n = T * F;
    const long row0 = (long)blockIdx.x * T;
    float part = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int t = i / F, f = i - t * F;
        const float v = a.a[(row0 + t) * a.lda + f] + a.x[(row0 + t) * a.Fs + f];
        buf[i] = v;
        part += v;
    }
    const float mean = (float)(block_sum<kThreads>((double)part, red) / n);
    part = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) {  // the values this thread wrote itself
        const float e = buf[i] - mean;
        part += e * e;
    }
    const float rs = gln_scale(block_sum<kThreads>((double)part, red) / n);
    for (int i = threadIdx.x; i < T * a.Fs; i += kThreads) {
        const int t = i / a.Fs, f = i - t * a.Fs;
        a.y[(row0 + t) * a.Fs + f] = f < F ? (buf[t * F + f] - mean) * rs * a.w[f] + a.b[f] : 0.f;
    }
}

// ---- odd layers -----------------------------------------------------------------------------------------------------------------------
struct Qkv5Args {
    const float *x;        // [S][5][T][Fs]
    const float *w[3], *b[3];  // ql / kl / vl: [5][5], [5]
    float *qkv;            // [S][F][T][16]
    int T, F, Fs;
};

__global__ __launch_bounds__(kThreads) void k_gtsa_qkv5(Qkv5Args a) {
    const int s = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.T * a.F) return;
    const int t = i / a.F, f = i - t * a.F;
    float xin[kC], o[16];
#pragma unroll
    for (int c = 0; c < kC; c++) xin[c] = a.x[(((long)s * kC + c) * a.T + t) * a.Fs + f];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int j = 0; j < kC; j++) {
            float v = a.b[p][j];
#pragma unroll
            for (int c = 0; c < kC; c++) v += a.w[p][j * kC + c] * xin[c];
            o[p * kC + j] = v;
        }
    o[15] = 0.f;
    float4 *dst = reinterpret_cast<float4 *>(a.qkv + (((long)s * a.F + f) * a.T + t) * 16);
#pragma unroll
    for (int p = 0; p < 4; p++) dst[p] = make_float4(o[4 * p], o[4 * p + 1], o[4 * p + 2], o[4 * p + 3]);
}

struct Tail5Args {
    const float *att;  // [S][F][T] rows at stride lda, 5 values
    const float *x;    // [S][5][T][Fs]
    float *y;          // [S][5][T][Fs] (may be x)
    const float *wo, *bo, *naw, *nab, *win, *bin, *wout, *bout, *niw, *nib;  // linear [5][5], norm_a, linear_in [fn][5], linear_out [5][fn], norm_i
    int lda, T, F, Fs, fn;
};

// gLN over the T x 5 values of the sequence a lane holds in v (rows t = wave + 4 k): per-thread partial, then the four waves in order
__device__ __forceinline__ void norm5(float (&v)[kRowsPerThread][kC], int T, int wave, int lane, float (*red)[64], const float *w, const float *b) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++)
        if (wave + kWaves * k < T) {
#pragma unroll
            for (int c = 0; c < kC; c++) part += v[k][c];
        }
    __syncthreads();
    red[wave][lane] = part;
    __syncthreads();
    const double n = (double)kC * T;
    const float mean = (float)(((double)red[0][lane] + (double)red[1][lane] + (double)red[2][lane] + (double)red[3][lane]) / n);
    part = 0.f;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++)
        if (wave + kWaves * k < T) {
#pragma unroll
            for (int c = 0; c < kC; c++) {
                const float e = v[k][c] - mean;
                part += e * e;
            }
        }
    __syncthreads();
    red[wave][lane] = part;
    __syncthreads();
    const float rs = gln_scale(((double)red[0][lane] + (double)red[1][lane] + (double)red[2][lane] + (double)red[3][lane]) / n);
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++)
#pragma unroll
        for (int c = 0; c < kC; c++) v[k][c] = (v[k][c] - mean) * rs * w[c] + b[c];
}

__global__ __launch_bounds__(kThreads) void k_gtsa_tail5(Tail5Args a) {
    static_assert(kWaves == 4, "norm5 adds four waves");
    __shared__ float red[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y, f = blockIdx.x * 64 + lane, T = a.T, F = a.F;
    const bool live = f < F;
    float v[kRowsPerThread][kC];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++) {
        const int t = wave + kWaves * k;
#pragma unroll
        for (int c = 0; c < kC; c++) v[k][c] = 0.f;
        if (t < T && live) {
            const float *ar = a.att + (((long)s * F + f) * T + t) * a.lda;
            float at[kC];
#pragma unroll
            for (int c = 0; c < kC; c++) at[c] = ar[c];
#pragma unroll
            for (int c = 0; c < kC; c++) {
                float o = a.bo[c];
#pragma unroll
                for (int e = 0; e < kC; e++) o += a.wo[c * kC + e] * at[e];
                v[k][c] = o + a.x[(((long)s * kC + c) * T + t) * a.Fs + f];
            }
        }
    }
    norm5(v, T, wave, lane, red, a.naw, a.nab);
    float acc[kRowsPerThread][kC];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; k++)
#pragma unroll
        for (int c = 0; c < kC; c++) acc[k][c] = a.bout[c] + v[k][c];
    for (int j = 0; j < a.fn; j++) {  // wave-uniform weights: the hidden unit j of every row this thread holds, then gone
        float wi[kC], wo[kC];
#pragma unroll
        for (int c = 0; c < kC; c++) { wi[c] = a.win[j * kC + c]; wo[c] = a.wout[(long)c * a.fn + j]; }
        const float bj = a.bin[j];
#pragma unroll
        for (int k = 0; k < kRowsPerThread; k++)
            if (wave + kWaves * k < T) {
                float hj = bj;
#pragma unroll
                for (int c = 0; c < kC; c++) hj += wi[c] * v[k][c];
                hj = fmaxf(hj, 0.f);
#pragma unroll
                for (int c = 0; c < kC; c++) acc[k][c] += wo[c] * hj;
            }
    }
    norm5(acc, T, wave, lane, red, a.niw, a.nib);
    if (f < a.Fs) {
#pragma unroll
        for (int k = 0; k < kRowsPerThread; k++) {
            const int t = wave + kWaves * k;
            if (t < T) {
#pragma unroll
                for (int c = 0; c < kC; c++) a.y[(((long)s * kC + c) * T + t) * a.Fs + f] = live ? acc[k][c] : 0.f;
            }
        }
    }
}

// ---- output stage ---------------------------------------------------------------------------------------------------------------------
struct GatherArgs {
    const float *x;    // [S][5][T][Fs]
    const float *buf;  // [B][5][2][Fs]: the last two frames of the window before this pass
    float *A;          // [S T][3 * 5][Fs]
    int B, T, Fs;
};

__global__ __launch_bounds__(kThreads) void k_gtsa_gather3(GatherArgs a) {
    const int row = blockIdx.x, kc = blockIdx.y, k = kc / kC, c = kc - k * kC;
    const int T = a.T, s = row / T, t = row - s * T, ts = t - 2 + k;
    const float *src;
    if (ts >= 0) src = a.x + (((long)s * kC + c) * T + ts) * a.Fs;
    else if (s >= a.B) src = a.x + (((long)(s - a.B) * kC + c) * T + T + ts) * a.Fs;  // the window before, same utterance
    else src = a.buf + (((long)s * kC + c) * 2 + 2 + ts) * a.Fs;
    float *dst = a.A + ((long)row * 3 * kC + kc) * a.Fs;
    for (int f = threadIdx.x; f < a.Fs; f += kThreads) dst[f] = src[f];
}

// chunk chains: the two-frame buffer a pass leaves behind is the last two frames of every stream's OWN last window of the pass
struct LastFramesArgs {
    const float *x;       // [Nc B][5][T][Fs]
    const float *buf_in;  // [B][5][2][Fs]
    float *buf_out;       // [B][5][2][Fs], not buf_in
    const long *cnt;      // [B], clamped to [0, Nc] here
    int Nc, B, T, Fs;
};

__global__ __launch_bounds__(kThreads) void k_gtsa_lastframes_rows(LastFramesArgs a) {
    const int b = blockIdx.x, cj = blockIdx.y, c = cj >> 1, j = cj & 1;
    const long n = a.cnt[b];
    const int own = n < 0 ? 0 : (n > a.Nc ? a.Nc : (int)n);
    const long o = (((long)b * kC + c) * 2 + j) * a.Fs;
    const float *src = own == 0 ? a.buf_in + o : a.x + ((((long)(own - 1) * a.B + b) * kC + c) * a.T + a.T - 2 + j) * a.Fs;
    for (int f = threadIdx.x; f < a.Fs; f += kThreads) a.buf_out[o + f] = src[f];
}

struct OutArgs {
    const float *g;      // rows [S T] at stride ldg: conv_trans output at column o, conv_gated at Co + o, Co = 2 F
    const float *nw, *nb;  // [Co]
    const float2 *spec;  // [S][M][T][F]
    float2 *Y;           // [S][T][F]
    float *tap;          // optional [S][Co][T]: the normalised mask before decompress_cIRM
    int ldg, M, T, F;
};

__device__ __forceinline__ float gated(const float *g, int Co, int o) { return g[o] * (1.0f / (1.0f + expf(-g[Co + o]))); }

__device__ __forceinline__ float decompress_cirm(float m) {  // utility.py:439-442
    m = m >= 9.9f ? 9.9f : (m <= -9.9f ? -9.9f : m);
    return -10.0f * logf((10.0f - m) / (10.0f + m));
}

__global__ __launch_bounds__(kThreads) void k_gtsa_out(OutArgs a) {
    __shared__ double red[kThreads];
    const int s = blockIdx.x, T = a.T, F = a.F, Co = 2 * F, n = T * Co;
    const float *g = a.g + (long)s * T * a.ldg;
    float part = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int t = i / Co, o = i - t * Co;
        part += gated(g + (long)t * a.ldg, Co, o);
    }
    const float mean = (float)(block_sum<kThreads>((double)part, red) / n);
    part = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int t = i / Co, o = i - t * Co;
        const float e = gated(g + (long)t * a.ldg, Co, o) - mean;
        part += e * e;
    }
    const float rs = gln_scale(block_sum<kThreads>((double)part, red) / n);
    for (int i = threadIdx.x; i < T * F; i += kThreads) {
        const int t = i / F, f = i - t * F;
        const float *gr = g + (long)t * a.ldg;
        const float mr = (gated(gr, Co, f) - mean) * rs * a.nw[f] + a.nb[f];
        const float mi = (gated(gr, Co, F + f) - mean) * rs * a.nw[F + f] + a.nb[F + f];
        if (a.tap) {
            a.tap[((long)s * Co + f) * T + t] = mr;
            a.tap[((long)s * Co + F + f) * T + t] = mi;
        }
        const float cr = decompress_cirm(mr), ci = decompress_cirm(mi);
        const float2 X = a.spec[((long)s * a.M * T + t) * F + f];
        a.Y[((long)s * T + t) * F + f] = make_float2(cr * X.x - ci * X.y, ci * X.x + cr * X.y);
    }
}

int launched(const char *what) {
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "%s launch failed", what);
}

int bad_geometry(const char *what, int S, int T, int F, int Fs) {
    if (S <= 0 || S > 65535) return se::train_fail(SE_ERR_ARG, "%s: %d streams per call (1 .. 65535)", what, S);
    if (T <= 0 || T > kMaxT) return se::train_fail(SE_ERR_ARG, "%s: %d frames per window (at most %d)", what, T, kMaxT);
    if (F <= 0 || Fs < F) return se::train_fail(SE_ERR_ARG, "%s: %d frequencies at row stride %d", what, F, Fs);
    return 0;
}

}  // namespace

extern "C" {

int se_gtsa_limits(int *max_frames, int *max_maxlen, int *max_norm_values) {
    if (max_frames) *max_frames = kMaxT;
    if (max_maxlen) *max_maxlen = kMaxLen;
    if (max_norm_values) *max_norm_values = kNormMax;
    return SE_OK;
}

int se_gtsa_feat(const float *spec, float *x, int S, int M, int T, int F, int Fs, void *stream) {
    if (!spec || !x || M <= 0) return se::train_fail(SE_ERR_ARG, "se_gtsa_feat: null / bad argument");
    if (int rc = bad_geometry("se_gtsa_feat", S, T, F, Fs)) return rc;
    FeatArgs a{reinterpret_cast<const float2 *>(spec), x, M, T, F, Fs};
    hipLaunchKernelGGL(k_gtsa_feat, dim3((T * Fs + kThreads - 1) / kThreads, S), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_feat");
}

int se_gtsa_attn(const float *q, const float *kn, const float *vn, const float *kc, const float *vc, float *out, const float *delta, int ldq,
                 int ldk, int ldo, int S, int B, int U, int Hh, int D, int T, int maxlen, int model_dim, void *stream) {
    if (!q || !kn || !vn || !kc || !vc || !out || !delta || U <= 0 || Hh <= 0 || model_dim <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: null / bad argument");
    if (B <= 0 || S <= 0 || S % B || S > 0x7fffffff / kMaxT) return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: %d streams are not whole windows of %d utterances", S, B);
    if (T <= 0 || T > kMaxT) return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: %d frames per window (at most %d)", T, kMaxT);
    if (maxlen < T || maxlen > kMaxLen) return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: maxlen = %d (the %d frames of a window .. %d)", maxlen, T, kMaxLen);
    if ((long)U * Hh > 65535) return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: %d x %d (sequence, head) pairs per stream (at most 65535)", U, Hh);
    if (ldq < Hh * D || ldk < Hh * D || ldo < Hh * D) return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: row strides %d / %d / %d hold %d heads of %d", ldq, ldk, ldo, Hh, D);
    AttnArgs a{q, kn, vn, kc, vc, out, delta, ldq, ldk, ldo, B, U, Hh, T, maxlen, sqrtf((float)model_dim)};
    const dim3 grid(S, U * Hh);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (D == 67) hipLaunchKernelGGL(k_gtsa_attn<67>, grid, dim3(kThreads), 0, st, a);
    else if (D == 5) hipLaunchKernelGGL(k_gtsa_attn<5>, grid, dim3(kThreads), 0, st, a);
    else return se::train_fail(SE_ERR_ARG, "se_gtsa_attn: head width %d (67 = 201 / 3 on even layers, 5 = 2 * 3 - 1 on odd layers)", D);
    return launched("se_gtsa_attn");
}

int se_gtsa_tape(const float *kn, const float *vn, const float *kc, const float *vc, float *ko, float *vo, int ldk, int Nc, int B, int U, int Hh,
                 int D, int T, int maxlen, void *stream) {
    if (!kn || !vn || !kc || !vc || !ko || !vo || ko == kc || vo == vc || Nc <= 0 || B <= 0 || U <= 0 || Hh <= 0 || D <= 0 || T <= 0 || maxlen <= 0 ||
        ldk < Hh * D)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_tape: null / bad argument (the new carried part is written out of place)");
    TapeArgs a{kn, vn, kc, vc, ko, vo, ldk, Nc, B, U, Hh, D, T, maxlen, (long)B * U * Hh * maxlen * D};
    hipLaunchKernelGGL(k_gtsa_tape, dim3((unsigned)((a.total + kThreads - 1) / kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_tape");
}

int se_gtsa_tape_rows(const float *kn, const float *vn, const float *kc, const float *vc, float *ko, float *vo, const int64_t *cnt, int ldk, int Nc,
                      int B, int U, int Hh, int D, int T, int maxlen, void *stream) {
    if (!kn || !vn || !kc || !vc || !ko || !vo || !cnt || ko == kc || vo == vc || Nc <= 0 || B <= 0 || U <= 0 || Hh <= 0 || D <= 0 || T <= 0 ||
        maxlen <= 0 || ldk < Hh * D)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_tape_rows: null / bad argument (the new carried part is written out of place)");
    TapeRowsArgs a{{kn, vn, kc, vc, ko, vo, ldk, Nc, B, U, Hh, D, T, maxlen, (long)B * U * Hh * maxlen * D}, reinterpret_cast<const long *>(cnt)};
    hipLaunchKernelGGL(k_gtsa_tape_rows, dim3((unsigned)((a.t.total + kThreads - 1) / kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_tape_rows");
}

int se_gtsa_addnorm(const float *a_, int lda, const float *x, float *y, const float *w, const float *b, int nseq, int T, int F, int Fs, void *stream) {
    if (!a_ || !x || !y || !w || !b || nseq <= 0 || T <= 0 || F <= 0 || Fs < F || lda < F) return se::train_fail(SE_ERR_ARG, "se_gtsa_addnorm: null / bad argument");
    if ((long)T * F > kNormMax) return se::train_fail(SE_ERR_ARG, "se_gtsa_addnorm: %d x %d values per sequence (at most %d)", T, F, kNormMax);
    NormArgs a{a_, x, y, w, b, lda, T, F, Fs};
    hipLaunchKernelGGL(k_gtsa_addnorm, dim3(nseq), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_addnorm");
}

int se_gtsa_qkv5(const float *x, const float *wq, const float *bq, const float *wk, const float *bk, const float *wv, const float *bv, float *qkv,
                 int S, int T, int F, int Fs, void *stream) {
    if (!x || !wq || !bq || !wk || !bk || !wv || !bv || !qkv) return se::train_fail(SE_ERR_ARG, "se_gtsa_qkv5: null argument");
    if (int rc = bad_geometry("se_gtsa_qkv5", S, T, F, Fs)) return rc;
    Qkv5Args a{x, {wq, wk, wv}, {bq, bk, bv}, qkv, T, F, Fs};
    hipLaunchKernelGGL(k_gtsa_qkv5, dim3((T * F + kThreads - 1) / kThreads, S), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_qkv5");
}

int se_gtsa_tail5(const float *att, int lda, const float *x, float *y, const float *wo, const float *bo, const float *naw, const float *nab,
                  const float *win, const float *bin, const float *wout, const float *bout, const float *niw, const float *nib, int S, int T, int F,
                  int Fs, int fn, void *stream) {
    if (!att || !x || !y || !wo || !bo || !naw || !nab || !win || !bin || !wout || !bout || !niw || !nib || lda < kC || fn <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_tail5: null / bad argument");
    if (int rc = bad_geometry("se_gtsa_tail5", S, T, F, Fs)) return rc;
    Tail5Args a{att, x, y, wo, bo, naw, nab, win, bin, wout, bout, niw, nib, lda, T, F, Fs, fn};
    hipLaunchKernelGGL(k_gtsa_tail5, dim3((Fs + 63) / 64, S), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_tail5");
}

int se_gtsa_gather3(const float *x, const float *buf, float *A, int S, int B, int T, int Fs, void *stream) {
    if (!x || !buf || !A || S <= 0 || B <= 0 || S % B || T < 2 || Fs <= 0 || (long)S * T > 0x7fffffff)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_gather3: null / bad argument (whole windows of B utterances, at least 2 frames)");
    GatherArgs a{x, buf, A, B, T, Fs};
    hipLaunchKernelGGL(k_gtsa_gather3, dim3(S * T, 3 * kC), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_gather3");
}

int se_gtsa_lastframes_rows(const float *x, const float *buf_in, float *buf_out, const int64_t *cnt, int Nc, int B, int T, int Fs, void *stream) {
    if (!x || !buf_in || !buf_out || !cnt || buf_out == buf_in || Nc <= 0 || B <= 0 || B > 0x7fffffff / Nc || T < 2 || Fs <= 0)
        return se::train_fail(SE_ERR_ARG, "se_gtsa_lastframes_rows: null / bad argument (out of place, at least 2 frames)");
    LastFramesArgs a{x, buf_in, buf_out, reinterpret_cast<const long *>(cnt), Nc, B, T, Fs};
    hipLaunchKernelGGL(k_gtsa_lastframes_rows, dim3(B, 2 * kC), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_lastframes_rows");
}

int se_gtsa_out(const float *g, int ldg, const float *nw, const float *nb, const float *spec, float *Y, float *tap, int S, int M, int T, int F,
                void *stream) {
    if (!g || !nw || !nb || !spec || !Y || S <= 0 || M <= 0 || T <= 0 || F <= 0 || ldg < 4 * F) return se::train_fail(SE_ERR_ARG, "se_gtsa_out: null / bad argument");
    OutArgs a{g, nw, nb, reinterpret_cast<const float2 *>(spec), reinterpret_cast<float2 *>(Y), tap, ldg, M, T, F};
    hipLaunchKernelGGL(k_gtsa_out, dim3(S), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    return launched("se_gtsa_out");
}

}  // extern "C"
