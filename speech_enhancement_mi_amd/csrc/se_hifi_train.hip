// HiFi-GAN generator training (speech_enhancement_mi_amd/hifigan_training.py is the caller): the backward kernels of what csrc/se_hifi.hip
// adds to the se_train_* convolutions / GEMMs.  fp32, no float atomics, every reduction in a fixed order that does not depend on the
// number of streams S; activations [S][C][T][F], S = windows x utterances, window-major (s = n B + b), as in se_hifi.hip.
//
//   k_hifi_lstm_bwd_step  one step of the LSTM's backward sweep, for ALL windows of a pass at once: the reference detaches (h, c) at
//                     every window seam, so the rows are the R = B Nc (utterance, window) pairs and the sweep is T steps long.  One
//                     workgroup per hidden unit j and 8 rows: dh_rec[j] = dgates[t + 1] . W_hh^T[j] over 4H, every thread a fixed
//                     stride of k, the wave by the fixed butterfly, the four waves summed as (0 + 1) + (2 + 3); then the unit's four
//                     gate gradients and the carried dc from the saved gates and cells.  A value of dgates[t + 1] is used once per
//                     workgroup, so it is read straight from memory (L2), not staged in LDS; no workgroup waits for another (one
//                     launch per step).  <true> (se_hifi_lstm_bwd_rows, chunk chains): row r = b Nc + n is swept only where
//                     n < live[b]; a dead row reads nothing, its dgates are exact zeros at every step, and a tile of 8 dead rows
//                     returns before the dot products.  A live row's arithmetic is the plain kernel's.
//   k_hifi_norm_esum / k_hifi_norm_bwd   the running-mean norm and the fc's tanh: e = dy w, d tanh = e - (1 - alpha_n) mean_{T x D}(e),
//                     do = d tanh (1 - tanh^2) in the fc's row layout [B][Nc T][D]; dw, db as [S][D] slabs (sums over t in order).
//                     <true> (se_hifi_seqnorm_bwd_rows): window n of utterance b is at step[b] + n D, and a window n >= cnt[b] reads
//                     neither dy nor o and writes zeros to its dout rows and its slabs
//   k_hifi_gate_bwd   dx = dy d/dx (tanh(x) sigmoid(x))
//   k_hifi_skip_bwd   the gated skip: d(u | v) stacked as the forward reads them, and d yd through the self-gate (the padded
//                     frequency columns f >= Fy receive nothing)
//   k_hifi_rows_bwd   the adjoint of k_hifi_rows (a permutation)
//   k_hifi_chansum    part[s][c] = the sum over T x F (double partial sums, fixed tree): bias gradients, folded over s by se_train_colsum
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/se_engine.h"

namespace se {
int train_fail(int code, const char *fmt, ...);  // se_train.hip (owns se_train_last_error)
}

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerWg = 8;

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float selfgate(float y) { return tanhf(y) * sigmoid_(y); }
// d/dy tanh(y) sigmoid(y) = sech^2(y) sigmoid(y) + tanh(y) sigmoid(y) (1 - sigmoid(y))
__device__ __forceinline__ float selfgate_grad(float y) {
    const float t = tanhf(y), s = sigmoid_(y);
    return (1.0f - t * t) * s + t * s * (1.0f - s);
}

struct LstmBwdArgs {
    const float *dout;    // [R][T][H], this step's column block: + t H
    const float *dgnext;  // dgates of step t + 1, [R][T][4H] + (t + 1) 4H; null at t = T - 1 (the detached seam: dh_rec = dc = 0)
    const float *whht;    // W_hh^T [H][4H]
    const float *gates;   // saved activated gates of step t
    const float *cs;      // saved cells [R T][H]: c_t at row r T + t
    const float *cprev;   // [R T][H]: c_{t-1} of every row - cs shifted by one step, the pass's entry cell in front of every utterance
    float *dg;            // dgates of step t
    float *dc;            // [R][H], the carried cell gradient; written at t = T - 1 before it is ever read
    int R, H, T, t;
    const int *live;      // kRows: [B], utterance b's own windows of this pass; row r = b Nc + n is dead where n >= live[b]
    int Nc;
};

__device__ __forceinline__ bool row_live(const LstmBwdArgs &a, int r) { return r % a.Nc < a.live[r / a.Nc]; }

template <bool kRows>
__global__ __launch_bounds__(kThreads) void k_hifi_lstm_bwd_step(LstmBwdArgs a) {
    __shared__ float red[4][kRowsPerWg];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = blockIdx.x, r0 = blockIdx.y * kRowsPerWg;
    const int nb = min(kRowsPerWg, a.R - r0);
    const int H4 = 4 * a.H;
    const long ldg = (long)a.T * H4;
    if (kRows) {
        bool any = false;   // the same for every thread of the workgroup
        for (int b = 0; b < nb; b++) any |= row_live(a, r0 + b);
        if ((int)threadIdx.x < nb && !row_live(a, r0 + threadIdx.x)) {
            float *dg = a.dg + ((long)(r0 + threadIdx.x) * a.T + a.t) * H4;
            dg[j] = 0.0f, dg[a.H + j] = 0.0f, dg[2 * a.H + j] = 0.0f, dg[3 * a.H + j] = 0.0f;
        }
        if (!any) return;   // all eight rows are dead: no dot products
    }
    if (a.dgnext) {
        const float *w = a.whht + (long)j * H4;
        const float *rows[kRowsPerWg];
#pragma unroll
        for (int b = 0; b < kRowsPerWg; b++) rows[b] = a.dgnext + (long)(r0 + min(b, nb - 1)) * ldg;   // past the batch: a valid row, never used
        float acc[kRowsPerWg];
#pragma unroll
        for (int b = 0; b < kRowsPerWg; b++) acc[b] = 0.0f;
        for (int k = threadIdx.x; k < H4; k += kThreads) {
            const float wv = w[k];
#pragma unroll
            for (int b = 0; b < kRowsPerWg; b++) acc[b] = fmaf(wv, rows[b][k], acc[b]);
        }
#pragma unroll
        for (int b = 0; b < kRowsPerWg; b++) {
            for (int off = 32; off > 0; off >>= 1) acc[b] += __shfl_xor(acc[b], off);
            if (lane == 0) red[wave][b] = acc[b];
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nb && (!kRows || row_live(a, r0 + threadIdx.x))) {
        const int b = threadIdx.x;
        const long r = r0 + b;
        const long row = r * a.T + a.t;   // the row of step t in the [R T][.] tensors
        float dh = a.dout[row * a.H + j], dc = 0.0f;
        if (a.dgnext) {
            dh += (red[0][b] + red[1][b]) + (red[2][b] + red[3][b]);
            dc = a.dc[r * a.H + j];
        }
        const float *g = a.gates + row * H4;
        const float ig = g[j], fg = g[a.H + j], gg = g[2 * a.H + j], og = g[3 * a.H + j];
        const float c = a.cs[row * a.H + j];
        const float cp = a.cprev[row * a.H + j];
        const float tc = tanhf(c);
        dc += dh * og * (1.0f - tc * tc);
        float *dg = a.dg + row * H4;
        dg[j] = dc * gg * ig * (1.0f - ig);
        dg[a.H + j] = dc * cp * fg * (1.0f - fg);
        dg[2 * a.H + j] = dc * ig * (1.0f - gg * gg);
        dg[3 * a.H + j] = dh * tc * og * (1.0f - og);
        a.dc[r * a.H + j] = dc * fg;
    }
}

// em[s] = mean over (c, t, f) of dy[s] w[c F + f]: per-thread double partial sums over a fixed stride, then a fixed tree
// kRows: stream s = n B + b is dead where n >= cnt[b] (clamped to 0 .. Nc, as k_hifi_scan_rows reads it): em[s] = 0, dy unread
template <bool kRows>
__global__ __launch_bounds__(kThreads) void k_hifi_norm_esum(const float *__restrict__ dy, const float *__restrict__ w, float *__restrict__ em,
                                                             const int64_t *__restrict__ cnt, int B, int C_, int T, int F) {
    __shared__ double part[kThreads];
    if (kRows) {
        const int nn = blockIdx.x / B, b = blockIdx.x - nn * B;
        if ((int64_t)nn >= cnt[b]) {   // the same for every thread of the workgroup
            if (threadIdx.x == 0) em[blockIdx.x] = 0.0f;
            return;
        }
    }
    const int n = C_ * T * F;
    const float *p = dy + (long)blockIdx.x * n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int f = i % F, c = i / (T * F);
        s += (double)(p[i] * w[c * F + f]);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) em[blockIdx.x] = (float)(part[0] / (double)n);
}

// one thread per (stream s, feature d), the T frames in order
template <bool kRows>
__global__ __launch_bounds__(kThreads) void k_hifi_norm_bwd(const float *__restrict__ dy, const float *__restrict__ o, const float *__restrict__ w,
                                                            const float *__restrict__ g, const float *__restrict__ em, double step,
                                                            const int64_t *__restrict__ step0, const int64_t *__restrict__ cnt, float *__restrict__ dout,
                                                            float *__restrict__ pw, float *__restrict__ pb, int Nc, int B, int C_, int T, int F) {
    const int D = C_ * F, d = blockIdx.x * kThreads + threadIdx.x;
    if (d >= D) return;
    const int s = blockIdx.y, nn = s / B, b = s - nn * B;
    const int c = d / F, f = d - c * F;
    const long w_ = (long)b * Nc + nn;
    if (kRows) {
        if ((int64_t)nn >= cnt[b]) {   // a dead window: zeros to its rows of dout and to its slabs, nothing read
            for (int t = 0; t < T; t++) dout[(w_ * T + t) * D + d] = 0.0f;
            pw[(long)s * D + d] = 0.0f;
            pb[(long)s * D + d] = 0.0f;
            return;
        }
        step = (double)step0[b];
    }
    const double stepn = step + (double)nn * (double)D;
    const float keep = (float)(1.0 - stepn / (stepn + (double)D));   // 1 - alpha_n
    const float sub = keep * em[s], wd = w[d], gm = g[w_];
    float aw = 0.0f, ab = 0.0f;
    for (int t = 0; t < T; t++) {
        const float dyv = dy[(((long)s * C_ + c) * T + t) * F + f];
        const long io = (w_ * T + t) * D + d;
        const float th = tanhf(o[io]);
        dout[io] = (dyv * wd - sub) * (1.0f - th * th);
        aw = fmaf(dyv, th - gm, aw);
        ab += dyv;
    }
    pw[(long)s * D + d] = aw;
    pb[(long)s * D + d] = ab;
}

__global__ __launch_bounds__(kThreads) void k_hifi_gate_bwd(const float *__restrict__ dy, const float *__restrict__ x, float *__restrict__ dx, long n) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) dx[i] = dy[i] * selfgate_grad(x[i]);
}

__global__ __launch_bounds__(kThreads) void k_hifi_skip_bwd(const float *__restrict__ dout, const float *__restrict__ yd, const float *__restrict__ uv,
                                                            float *__restrict__ duv, float *__restrict__ dyd, long n, int Co, int T, int Fy, int Fr) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int f = (int)(i % Fr);
    const long rest = i / Fr;
    const int t = (int)(rest % T);
    const long sc = rest / T;
    const int c = (int)(sc % Co);
    const long s = sc / Co;
    const long iu = (((s * 2 + 0) * Co + c) * T + t) * Fr + f, iv = (((s * 2 + 1) * Co + c) * T + t) * Fr + f;
    const long iy = (sc * T + t) * Fy + f;
    const float ydv = f < Fy ? yd[iy] : 0.0f;
    const float z = f < Fy ? selfgate(ydv) : 0.0f;
    const float m = sigmoid_(uv[iv]), tu = tanhf(uv[iu]), go = dout[i];
    duv[iu] = go * m * (1.0f - tu * tu);
    duv[iv] = go * (tu - z) * m * (1.0f - m);
    if (f < Fy) dyd[iy] = go * (1.0f - m) * selfgate_grad(ydv);
}

__global__ __launch_bounds__(kThreads) void k_hifi_rows_bwd(const float *__restrict__ drows, float *__restrict__ dx, long n, int Nc, int B, int C_, int T, int F) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int D = C_ * F;
    const int d = (int)(i % D);
    const long row = i / D;
    const int t = (int)(row % T);
    const long bn = row / T;
    const int nn = (int)(bn % Nc), b = (int)(bn / Nc);
    const int c = d / F, f = d - c * F;
    dx[((((long)nn * B + b) * C_ + c) * T + t) * F + f] = drows[i];
}

__global__ __launch_bounds__(kThreads) void k_hifi_chansum(const float *__restrict__ x, float *__restrict__ part, int X) {
    __shared__ double acc[kThreads];
    const float *p = x + (long)blockIdx.x * X;
    double s = 0.0;
    for (int i = threadIdx.x; i < X; i += kThreads) s += (double)p[i];
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) acc[threadIdx.x] += acc[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = (float)acc[0];
}

int launched(const char *what) {
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "%s launch failed", what);
}

int blocks_of(const char *what, long n, unsigned *blocks) {
    const long nb = (n + kThreads - 1) / kThreads;
    if (n <= 0 || nb > 0x7fffffffL) return se::train_fail(SE_ERR_ARG, "%s: %ld elements (1 .. 2^31 - 1 workgroups of %d)", what, n, kThreads);
    *blocks = (unsigned)nb;
    return SE_OK;
}

// live = null: every row is swept (k_hifi_lstm_bwd_step<false>, which never reads a.live / a.Nc)
int lstm_bwd_launch(const char *what, const float *dout, const float *gates, const float *cs, const float *cprev, const float *whht, float *dgates, float *dc,
                    const int *live, int B, int Nc, int T, int H, void *stream) {
    if (!dout || !gates || !cs || !cprev || !whht || !dgates || !dc) return se::train_fail(SE_ERR_ARG, "%s: null argument", what);
    const long R = (long)B * Nc;
    if (B <= 0 || Nc <= 0 || T <= 0 || H < 8 || H % 8 || H > 1024 || (R + kRowsPerWg - 1) / kRowsPerWg > 65535)
        return se::train_fail(SE_ERR_ARG, "%s: %d utterances x %d windows of %d steps, hidden %d (a multiple of 8, up to 1024; up to %d rows)", what, B, Nc,
                              T, H, 65535 * kRowsPerWg);
    const dim3 grid(H, (unsigned)((R + kRowsPerWg - 1) / kRowsPerWg));
    for (int t = T - 1; t >= 0; t--) {
        LstmBwdArgs a;
        a.dout = dout, a.gates = gates, a.cs = cs, a.cprev = cprev, a.whht = whht, a.dg = dgates, a.dc = dc;
        a.dgnext = t == T - 1 ? nullptr : dgates + (long)(t + 1) * 4 * H;
        a.R = (int)R, a.H = H, a.T = T, a.t = t;
        a.live = live, a.Nc = Nc;
        if (live)
            hipLaunchKernelGGL(k_hifi_lstm_bwd_step<true>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
        else
            hipLaunchKernelGGL(k_hifi_lstm_bwd_step<false>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
    }
    return launched(what);
}

// step0 / cnt = null: one step for all and every window live (the <false> kernels, which never read the tables)
int seqnorm_bwd_launch(const char *what, const float *dy, const float *o, const float *w, const float *wm, double step, const int64_t *step0, const int64_t *cnt,
                       float *em, float *dout, float *pw, float *pb, int Nc, int B, int C_, int T, int F, void *stream) {
    if (!dy || !o || !w || !wm || !em || !dout || !pw || !pb) return se::train_fail(SE_ERR_ARG, "%s: null argument", what);
    if (Nc <= 0 || B <= 0 || (long)Nc * B > 65535 || C_ <= 0 || T <= 0 || F <= 0 || (long)T * C_ * F > (1L << 30) || step < 0.0)
        return se::train_fail(SE_ERR_ARG, "%s: bad geometry (%d windows x %d utterances <= 65535, C %d, T %d, F %d, step %g)", what, Nc, B, C_, T, F, step);
    const int D = C_ * F;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((D + kThreads - 1) / kThreads, Nc * B);
    if (cnt) {
        hipLaunchKernelGGL(k_hifi_norm_esum<true>, dim3(Nc * B), dim3(kThreads), 0, st, dy, w, em, cnt, B, C_, T, F);
        hipLaunchKernelGGL(k_hifi_norm_bwd<true>, grid, dim3(kThreads), 0, st, dy, o, w, wm, em, step, step0, cnt, dout, pw, pb, Nc, B, C_, T, F);
    } else {
        hipLaunchKernelGGL(k_hifi_norm_esum<false>, dim3(Nc * B), dim3(kThreads), 0, st, dy, w, em, cnt, B, C_, T, F);
        hipLaunchKernelGGL(k_hifi_norm_bwd<false>, grid, dim3(kThreads), 0, st, dy, o, w, wm, em, step, step0, cnt, dout, pw, pb, Nc, B, C_, T, F);
    }
    return launched(what);
}

}  // namespace

extern "C" {

int se_hifi_lstm_bwd(const float *dout, const float *gates, const float *cs, const float *cprev, const float *whht, float *dgates, float *dc, int B, int Nc, int T,
                     int H, void *stream) {
    return lstm_bwd_launch("se_hifi_lstm_bwd", dout, gates, cs, cprev, whht, dgates, dc, nullptr, B, Nc, T, H, stream);
}

int se_hifi_lstm_bwd_rows(const float *dout, const float *gates, const float *cs, const float *cprev, const float *whht, float *dgates, float *dc, const int *live,
                          int B, int Nc, int T, int H, void *stream) {
    if (!live) return se::train_fail(SE_ERR_ARG, "se_hifi_lstm_bwd_rows: null argument");
    return lstm_bwd_launch("se_hifi_lstm_bwd_rows", dout, gates, cs, cprev, whht, dgates, dc, live, B, Nc, T, H, stream);
}

int se_hifi_seqnorm_bwd(const float *dy, const float *o, const float *w, const float *wm, double step, float *em, float *dout, float *pw, float *pb, int Nc, int B,
                        int C_, int T, int F, void *stream) {
    return seqnorm_bwd_launch("se_hifi_seqnorm_bwd", dy, o, w, wm, step, nullptr, nullptr, em, dout, pw, pb, Nc, B, C_, T, F, stream);
}

int se_hifi_seqnorm_bwd_rows(const float *dy, const float *o, const float *w, const float *wm, const int64_t *step, const int64_t *cnt, float *em, float *dout,
                             float *pw, float *pb, int Nc, int B, int C_, int T, int F, void *stream) {
    if (!step || !cnt) return se::train_fail(SE_ERR_ARG, "se_hifi_seqnorm_bwd_rows: null argument");
    return seqnorm_bwd_launch("se_hifi_seqnorm_bwd_rows", dy, o, w, wm, 0.0, step, cnt, em, dout, pw, pb, Nc, B, C_, T, F, stream);
}

int se_hifi_gate_bwd(const float *dy, const float *x, float *dx, int64_t n, void *stream) {
    if (!dy || !x || !dx) return se::train_fail(SE_ERR_ARG, "se_hifi_gate_bwd: null argument");
    unsigned nb;
    if (int rc = blocks_of("se_hifi_gate_bwd", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_gate_bwd, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), dy, x, dx, n);
    return launched("se_hifi_gate_bwd");
}

int se_hifi_skip_bwd(const float *dout, const float *yd, const float *uv, float *duv, float *dyd, int S, int Co, int T, int Fy, int Fr, void *stream) {
    if (!dout || !yd || !uv || !duv || !dyd) return se::train_fail(SE_ERR_ARG, "se_hifi_skip_bwd: null argument");
    if (S <= 0 || Co <= 0 || T <= 0 || Fy <= 0 || Fr < Fy)
        return se::train_fail(SE_ERR_ARG, "se_hifi_skip_bwd: bad geometry (S %d, Co %d, T %d, Fy %d <= Fr %d)", S, Co, T, Fy, Fr);
    const long n = (long)S * Co * T * Fr;
    unsigned nb;
    if (int rc = blocks_of("se_hifi_skip_bwd", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_skip_bwd, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), dout, yd, uv, duv, dyd, n, Co, T, Fy, Fr);
    return launched("se_hifi_skip_bwd");
}

int se_hifi_rows_bwd(const float *drows, float *dx, int Nc, int B, int C_, int T, int F, void *stream) {
    if (!drows || !dx) return se::train_fail(SE_ERR_ARG, "se_hifi_rows_bwd: null argument");
    if (Nc <= 0 || B <= 0 || C_ <= 0 || T <= 0 || F <= 0) return se::train_fail(SE_ERR_ARG, "se_hifi_rows_bwd: bad geometry");
    const long n = (long)Nc * B * C_ * T * F;
    unsigned nb;
    if (int rc = blocks_of("se_hifi_rows_bwd", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_rows_bwd, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), drows, dx, n, Nc, B, C_, T, F);
    return launched("se_hifi_rows_bwd");
}

int se_hifi_chansum(const float *x, float *part, int64_t rows, int X, void *stream) {
    if (!x || !part) return se::train_fail(SE_ERR_ARG, "se_hifi_chansum: null argument");
    if (rows <= 0 || rows > 0x7fffffffL || X <= 0) return se::train_fail(SE_ERR_ARG, "se_hifi_chansum: %ld rows of %d values", (long)rows, X);
    hipLaunchKernelGGL(k_hifi_chansum, dim3((unsigned)rows), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, part, X);
    return launched("se_hifi_chansum");
}

}  // extern "C"
