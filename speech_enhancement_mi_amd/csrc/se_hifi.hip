// HiFi-GAN generator inference (reference Hifi-GAN/hifigan.py:444-656; speech_enhancement_mi_amd/hifigan.py is the caller): what the
// generator needs beyond the se_train_* convolutions / GEMM and the se_sig_* signal chain.  fp32 throughout, no float atomics, every
// reduction in a fixed order that does not depend on the number of streams S; activations [S][C][T][F], S = windows x utterances,
// window-major (s = n B + b).
//
//   k_hifi_postnet    the hot path: twelve 1x1 convolutions (2 -> 128, ten of 128 -> 128, 128 -> 2) with the self-gate
//                     tanh(y) * sigmoid(y) after each.  A workgroup owns 128 bins of ONE stream and runs all twelve layers on them:
//                     the [128 channels][128 bins] activation stays in LDS (65 KiB: two workgroups per CU, one's epilogue under the
//                     other's MFMAs), each 128 x 128 weight is read once per layer and workgroup, straight into the A-fragment
//                     registers of the wave that owns its rows and one layer ahead, the ten inner layers run on
//                     v_mfma_f32_32x32x2_f32 (exact f32; wave w owns output channels [32 w, 32 w + 32) of all four 32-bin blocks,
//                     64 accumulator registers), bias + self-gate (fastgate: one exponential, one division) are the epilogue, the
//                     first and the last layer run on the vector ALU, and only the final two channels are written.  Bins past
//                     the end of the stream compute on zeros and are never stored.
//   k_hifi_gate       y = tanh(x) * sigmoid(x), pointwise (after the encoder convolutions and the last transposed convolution)
//   k_hifi_skip       the decoder's gated skip without a norm: out = sigmoid(v) tanh(u) + (1 - sigmoid(v)) z, z = self-gate of the
//                     transposed convolution's output zero-padded in F to the skip tensor, (u, v) = the stacked 1x1 pair
//   k_hifi_rows       [S][C][T][F] -> the LSTM's rows [B][Nc T][C F]
//   k_hifi_lstm_step  one LSTM time step: gates = gi[t] + h W_hh^T, then the cell update.  One workgroup per hidden unit and 8 batch
//                     rows (its h rows staged in LDS once), one wave per gate, the dot products reduced across the wave by a fixed butterfly; no
//                     workgroup waits for another (one launch per step; it re-reads W_hh every step)
//   k_hifi_winmean / k_hifi_scan / k_hifi_normapply   the bottleneck's tanh and running-mean norm: the mean of tanh(o) over T x D per
//                     window (double partial sums, fixed tree), the per-utterance scan g = alpha g + (1 - alpha) mean with
//                     alpha = step / (step + D) in double, and y = (tanh(o) - g) w + b written back in [S][C][T][F]
//   k_hifi_lstm_step<.., true>   training (se_hifi_lstm_train_fwd): the step also stores its activated gates and cell; the backward
//                     kernels are csrc/se_hifi_train.hip
//   k_hifi_lstm_step<true> / k_hifi_scan_rows   chunk chains (se_hifi_lstm_rows, se_hifi_seqnorm_rows): every row its own number of
//                     steps, every utterance its own window count and its own step; a row's arithmetic is the plain kernels'
//   k_hifi_lstm_step<true, true>   chunk-chain training (se_hifi_lstm_train_fwd_rows): both at once, and a finished row's step stores
//                     zeros as its gates and cell, so whatever the backward reads of them is finite
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/se_engine.h"

namespace se {
int train_fail(int code, const char *fmt, ...);  // se_train.hip (owns se_train_last_error)
}

namespace {

constexpr int kThreads = 256;
constexpr int kPC = 128;                       // postnet channels
constexpr int kPB = 128;                       // bins per workgroup
constexpr int kPostLayers = 12;
constexpr int kInner = kPC * kPC + kPC;        // floats of one inner layer in the pack: weight, bias
constexpr int kPackFirst = 2 * kPC + kPC;      // layer 0: weight [128][2], bias
constexpr int kPackLast = kPackFirst + (kPostLayers - 2) * kInner;
constexpr size_t kPostLds = (size_t)(kPC * kPB + 2 * kPB) * sizeof(float);   // two workgroups per CU
constexpr int kLstmBT = 8;                     // batch rows per workgroup of the LSTM step

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float selfgate(float y) { return tanhf(y) * sigmoid_(y); }

// tanh(y) sigmoid(y) from ONE exponential and one division: with t = exp(-|y|), tanh(|y|) = (1 - t^2) / (1 + t^2) and
// sigmoid(|y|) = 1 / (1 + t), so the gate is (1 - t) / (1 + t^2) for y >= 0 and -t (1 - t) / (1 + t^2) for y < 0.  Absolute error about
// 1e-7 (the cancellation in 1 - t near y = 0 is absolute, not relative); the postnet's epilogue runs it 64 times per lane and layer,
// where tanhf + expf + a division cost as much as the layer's MFMAs.
__device__ __forceinline__ float fastgate(float y) {
    const float t = __expf(-fabsf(y));
    const float q = __fdividef(1.0f - t, fmaf(t, t, 1.0f));
    return y >= 0.0f ? q : -t * q;
}

__global__ __launch_bounds__(kThreads, 2) void k_hifi_postnet(const float *__restrict__ x, const float *__restrict__ pack, float *__restrict__ y, int nbins) {
    extern __shared__ float lds[];
    float *X = lds, *xin = X + kPC * kPB;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, kh = lane >> 5;
    const int bin0 = blockIdx.x * kPB;
    const float *xs = x + (long)blockIdx.y * 2 * nbins;
    float *ys = y + (long)blockIdx.y * 2 * nbins;
    // The A fragments of a layer, straight from memory into registers: MFMA step j of lane half kh contracts k = 64 kh + j (any
    // assignment of k to steps is a valid one as long as A and B agree), so a lane holds 64 consecutive floats of its weight row and
    // every weight is read once per layer and workgroup.
    float4 wreg[16];
    const float *wlane = pack + kPackFirst + (32 * wave + r) * kPC + 64 * kh;
#pragma unroll
    for (int i = 0; i < 16; i++) wreg[i] = reinterpret_cast<const float4 *>(wlane)[i];
    {
        const int o = tid / kPB, b = tid % kPB;
        xin[tid] = bin0 + b < nbins ? xs[(long)o * nbins + bin0 + b] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < kPC * kPB; i += kThreads) {   // layer 0: 2 -> 128
        const int o = i / kPB, b = i % kPB;
        X[i] = fastgate(fmaf(pack[2 * o + 1], xin[kPB + b], pack[2 * o] * xin[b]) + pack[2 * kPC + o]);
    }
    const float *xcol = X + 64 * kh * kPB + r;
    for (int layer = 1; layer < kPostLayers - 1; layer++) {
        const float *bg = pack + kPackFirst + (layer - 1) * kInner + kPC * kPC;
        __syncthreads();   // X of the previous layer written
        f32x16 acc[kPB / 32];
#pragma unroll
        for (int nb = 0; nb < kPB / 32; nb++)
            for (int e = 0; e < 16; e++) acc[nb][e] = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float a4[4] = {wreg[i].x, wreg[i].y, wreg[i].z, wreg[i].w};
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int nb = 0; nb < kPB / 32; nb++)
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], xcol[(4 * i + e) * kPB + nb * 32], acc[nb], 0, 0, 0);
        }
        if (layer + 1 < kPostLayers - 1) {   // the next layer's fragments travel under the epilogue
#pragma unroll
            for (int i = 0; i < 16; i++) wreg[i] = reinterpret_cast<const float4 *>(wlane + layer * kInner)[i];
        }
        __syncthreads();   // every read of X done: X takes the layer's output
#pragma unroll
        for (int nb = 0; nb < kPB / 32; nb++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int o = 32 * wave + (e & 3) + 8 * (e >> 2) + 4 * kh;
                X[o * kPB + nb * 32 + r] = fastgate(acc[nb][e] + bg[o]);
            }
    }
    __syncthreads();
    {   // last layer: 128 -> 2
        const int o = tid / kPB, b = tid % kPB;
        const float *wl = pack + kPackLast + o * kPC;
        float sum = 0.0f;
        for (int c = 0; c < kPC; c++) sum = fmaf(wl[c], X[c * kPB + b], sum);
        if (bin0 + b < nbins) ys[(long)o * nbins + bin0 + b] = fastgate(sum + pack[kPackLast + 2 * kPC + o]);
    }
}

__global__ __launch_bounds__(kThreads) void k_hifi_gate(const float *__restrict__ x, float *__restrict__ y, long n) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) y[i] = selfgate(x[i]);
}

__global__ __launch_bounds__(kThreads) void k_hifi_skip(const float *__restrict__ yd, const float *__restrict__ uv, float *__restrict__ out, long n, int Co, int T,
                                                        int Fy, int Fr) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int f = (int)(i % Fr);
    const long rest = i / Fr;
    const int t = (int)(rest % T);
    const long sc = rest / T;
    const int c = (int)(sc % Co);
    const long s = sc / Co;
    const long iu = (((s * 2 + 0) * Co + c) * T + t) * Fr + f, iv = (((s * 2 + 1) * Co + c) * T + t) * Fr + f;
    const float z = f < Fy ? selfgate(yd[(sc * T + t) * Fy + f]) : 0.0f;
    const float m = sigmoid_(uv[iv]);
    out[i] = m * tanhf(uv[iu]) + (1.0f - m) * z;
}

__global__ __launch_bounds__(kThreads) void k_hifi_rows(const float *__restrict__ x, float *__restrict__ rows, long n, int Nc, int B, int C_, int T, int F) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int D = C_ * F;
    const int d = (int)(i % D);
    const long row = i / D;
    const int t = (int)(row % T);
    const long bn = row / T;
    const int nn = (int)(bn % Nc), b = (int)(bn / Nc);
    const int c = d / F, f = d - c * F;
    rows[i] = x[((((long)nn * B + b) * C_ + c) * T + t) * F + f];
}

struct LstmArgs {
    const float *gi, *hin, *cin, *whh;
    float *out, *cout, *hT;
    long ldgi, ldh, ldo;
    int B, H;
    const int *steps;   // kRows: row b runs steps[b] steps, this launch is step t of them
    int t;
    float *gates, *cs;  // kSave: this step's activated gates (i, f, g, o) and cell, rows at ldg / ldc
    long ldg, ldc;
};

// kRows (chunk chains): a row is live at step t while t < steps[row].  A live row computes what it computes in the plain kernel - the
// dot products of a row never see another row's h - and a finished one writes a zero into out[row][t] (the fc GEMM and the window
// means read all of out), at t = 0 also its h0 / c0 into hT / cT (steps = 0).  The last live step of a row writes its hT.
// kSave (training, se_hifi_lstm_train_fwd): the same arithmetic, and the step's activated gates and cell are stored for the backward.
// Both (se_hifi_lstm_train_fwd_rows): a finished row's step stores zeros as its gates and cell - the backward's shifted cell tensor and
// the weight-gradient GEMMs read every row of the workspace.
template <bool kRows, bool kSave>
__global__ __launch_bounds__(kThreads) void k_hifi_lstm_step(LstmArgs a) {
    __shared__ float pre[4][kLstmBT];
    extern __shared__ float hs[];   // [kLstmBT][H]: the batch tile's h rows, read from memory once per workgroup, zeros past the batch
    const int gate = threadIdx.x >> 6, lane = threadIdx.x & 63;   // wave g: gate g (i, f, g, o) of hidden unit j for 8 batch rows
    const int j = blockIdx.x, b0 = blockIdx.y * kLstmBT;
    const int nb = min(kLstmBT, a.B - b0);
    if (kRows) {
        bool any = false;   // the same for every thread of the workgroup
        for (int b = 0; b < nb; b++) any |= a.t < a.steps[b0 + b];
        if ((int)threadIdx.x < nb && a.t >= a.steps[b0 + threadIdx.x]) {
            const long row = b0 + threadIdx.x;
            a.out[row * a.ldo + j] = 0.0f;
            if (kSave) {
                float *g = a.gates + row * a.ldg;
                g[j] = 0.0f, g[a.H + j] = 0.0f, g[2 * a.H + j] = 0.0f, g[3 * a.H + j] = 0.0f;
                a.cs[row * a.ldc + j] = 0.0f;
            }
            if (a.t == 0) {
                a.hT[row * a.H + j] = a.hin[row * a.ldh + j];
                a.cout[row * a.H + j] = a.cin[row * a.H + j];
            }
        }
        if (!any) return;   // all eight rows have finished: nothing to stage
    }
    for (int i = threadIdx.x; i < kLstmBT * a.H; i += kThreads) {
        const int b = i / a.H, k = i - b * a.H;
        hs[i] = b < nb && (!kRows || a.t < a.steps[b0 + b]) ? a.hin[(long)(b0 + b) * a.ldh + k] : 0.0f;
    }
    __syncthreads();
    const float *w = a.whh + ((long)gate * a.H + j) * a.H;
    float acc[kLstmBT];
#pragma unroll
    for (int b = 0; b < kLstmBT; b++) acc[b] = 0.0f;
    for (int k = lane; k < a.H; k += 64) {
        const float wv = w[k];
#pragma unroll
        for (int b = 0; b < kLstmBT; b++) acc[b] = fmaf(wv, hs[b * a.H + k], acc[b]);
    }
#pragma unroll
    for (int b = 0; b < kLstmBT; b++) {
        for (int off = 32; off > 0; off >>= 1) acc[b] += __shfl_xor(acc[b], off);
        if (lane == 0) pre[gate][b] = acc[b];
    }
    __syncthreads();
    if ((int)threadIdx.x < nb && (!kRows || a.t < a.steps[b0 + threadIdx.x])) {
        const int b = threadIdx.x;
        const long row = b0 + b;
        const float *gi = a.gi + row * a.ldgi;
        const float ig = sigmoid_(gi[j] + pre[0][b]), fg = sigmoid_(gi[a.H + j] + pre[1][b]);
        const float gg = tanhf(gi[2 * a.H + j] + pre[2][b]), og = sigmoid_(gi[3 * a.H + j] + pre[3][b]);
        const float c = fg * a.cin[row * a.H + j] + ig * gg;
        const float h = og * tanhf(c);
        a.cout[row * a.H + j] = c;
        a.out[row * a.ldo + j] = h;
        if (kSave) {
            float *g = a.gates + row * a.ldg;
            g[j] = ig, g[a.H + j] = fg, g[2 * a.H + j] = gg, g[3 * a.H + j] = og;
            a.cs[row * a.ldc + j] = c;
        }
        if (kRows ? a.t == a.steps[row] - 1 : a.hT != nullptr) a.hT[row * a.H + j] = h;
    }
}

// wm[b Nc + n] = mean over T x D of tanh(o[b][n]): per-thread double partial sums over a fixed stride, then a fixed tree
__global__ __launch_bounds__(kThreads) void k_hifi_winmean(const float *__restrict__ o, float *__restrict__ wm, int TD) {
    __shared__ double part[kThreads];
    const float *p = o + (long)blockIdx.x * TD;
    double s = 0.0;
    for (int i = threadIdx.x; i < TD; i += kThreads) s += (double)tanhf(p[i]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) wm[blockIdx.x] = (float)(part[0] / (double)TD);
}

// per utterance: the running mean after each of the pass's windows, in place over the window means; torch's float32 arithmetic
// (alpha and 1 - alpha formed in double, rounded to float, two products and a sum)
__global__ void k_hifi_scan(float *__restrict__ wm, const float *__restrict__ mean_in, float *__restrict__ mean_out, double step, int B, int Nc, int D) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float g = mean_in[b];
    for (int n = 0; n < Nc; n++) {
        const double alpha = step / (step + (double)D);
        g = __fadd_rn(__fmul_rn((float)alpha, g), __fmul_rn((float)(1.0 - alpha), wm[b * Nc + n]));
        wm[b * Nc + n] = g;
        step += (double)D;
    }
    mean_out[b] = g;
}

// chunk chains: utterance b scans its own first cnt[b] windows from its own step[b]; a window past them receives the utterance's
// last running mean (finite values for k_hifi_normapply, which nothing reads), and cnt[b] = 0 hands mean_in[b] on
__global__ void k_hifi_scan_rows(float *__restrict__ wm, const float *__restrict__ mean_in, float *__restrict__ mean_out, const int64_t *__restrict__ step0,
                                 const int64_t *__restrict__ cnt, int B, int Nc, int D) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float g = mean_in[b];
    double step = (double)step0[b];
    const int64_t c = cnt[b];
    const int own = c < 0 ? 0 : c > Nc ? Nc : (int)c;
    for (int n = 0; n < Nc; n++) {
        if (n < own) {
            const double alpha = step / (step + (double)D);
            g = __fadd_rn(__fmul_rn((float)alpha, g), __fmul_rn((float)(1.0 - alpha), wm[b * Nc + n]));
            step += (double)D;
        }
        wm[b * Nc + n] = g;
    }
    mean_out[b] = g;
}

__global__ __launch_bounds__(kThreads) void k_hifi_normapply(const float *__restrict__ o, const float *__restrict__ g, const float *__restrict__ w,
                                                             const float *__restrict__ bias, float *__restrict__ y, int Nc, int B, int C_, int T, int F) {
    const int D = C_ * F, i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= T * D) return;
    const int s = blockIdx.y, nn = s / B, b = s - nn * B;
    const int t = i / D, d = i - t * D, c = d / F, f = d - c * F;
    const long w_ = (long)b * Nc + nn;
    y[(((long)s * C_ + c) * T + t) * F + f] = (tanhf(o[(w_ * T + t) * D + d]) - g[w_]) * w[d] + bias[d];
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

// one launch per step; steps = null: every row runs all TT steps (k_hifi_lstm_step<false>, which never reads a.steps / a.t)
// gates / cs given (both): the training forward, which also stores gates [B][TT][4H] and cs [B][TT][H]
int lstm_launch(const char *what, const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, const int *steps,
                int B, int TT, int H, void *stream, float *gates = nullptr, float *cs = nullptr) {
    if (!gi || !h0 || !c0 || !whh || !out || !hT || !cT) return se::train_fail(SE_ERR_ARG, "%s: null argument", what);
    if (B <= 0 || (B + kLstmBT - 1) / kLstmBT > 65535 || TT <= 0 || H < 8 || H % 8 || H > 1024)
        return se::train_fail(SE_ERR_ARG, "%s: B = %d rows, %d steps, hidden %d (a multiple of 8, up to 1024)", what, B, TT, H);
    const dim3 grid(H, (B + kLstmBT - 1) / kLstmBT);
    for (int t = 0; t < TT; t++) {
        LstmArgs a;
        a.gi = gi + (long)t * 4 * H, a.ldgi = (long)TT * 4 * H;
        a.hin = t ? out + (long)(t - 1) * H : h0, a.ldh = t ? (long)TT * H : H;
        a.cin = t ? cT : c0, a.cout = cT;   // a cell is read and written by one lane only: in place from the second step on
        a.whh = whh, a.out = out + (long)t * H, a.ldo = (long)TT * H;
        a.hT = steps || t == TT - 1 ? hT : nullptr;
        a.B = B, a.H = H;
        a.steps = steps, a.t = t;
        a.gates = gates ? gates + (long)t * 4 * H : nullptr, a.ldg = (long)TT * 4 * H;
        a.cs = cs ? cs + (long)t * H : nullptr, a.ldc = (long)TT * H;
        if (steps && gates)
            hipLaunchKernelGGL((k_hifi_lstm_step<true, true>), grid, dim3(kThreads), (size_t)kLstmBT * H * sizeof(float), static_cast<hipStream_t>(stream), a);
        else if (steps)
            hipLaunchKernelGGL((k_hifi_lstm_step<true, false>), grid, dim3(kThreads), (size_t)kLstmBT * H * sizeof(float), static_cast<hipStream_t>(stream), a);
        else if (gates)
            hipLaunchKernelGGL((k_hifi_lstm_step<false, true>), grid, dim3(kThreads), (size_t)kLstmBT * H * sizeof(float), static_cast<hipStream_t>(stream), a);
        else
            hipLaunchKernelGGL((k_hifi_lstm_step<false, false>), grid, dim3(kThreads), (size_t)kLstmBT * H * sizeof(float), static_cast<hipStream_t>(stream), a);
    }
    return launched(what);
}

}  // namespace

extern "C" {

int se_hifi_postnet(const float *x, const float *pack, float *y, int S, int T, int F, void *stream) {
    if (!x || !pack || !y) return se::train_fail(SE_ERR_ARG, "se_hifi_postnet: null argument");
    if (S <= 0 || S > 65535 || T <= 0 || F <= 0 || (long)T * F > (1L << 24))
        return se::train_fail(SE_ERR_ARG, "se_hifi_postnet: S = %d streams (1 .. 65535) of T x F = %d x %d bins (up to 2^24)", S, T, F);
    static thread_local int attr_dev = -1;   // the dynamic-LDS opt-in is per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return se::train_fail(SE_ERR_HIP, "se_hifi_postnet: no HIP device");
    if (dev != attr_dev) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_hifi_postnet), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPostLds) != hipSuccess)
            return se::train_fail(SE_ERR_HIP, "se_hifi_postnet: %zu bytes of LDS refused", kPostLds);
        attr_dev = dev;
    }
    const int nbins = T * F;
    hipLaunchKernelGGL(k_hifi_postnet, dim3((nbins + kPB - 1) / kPB, S), dim3(kThreads), kPostLds, static_cast<hipStream_t>(stream), x, pack, y, nbins);
    return launched("se_hifi_postnet");
}

int se_hifi_gate(const float *x, float *y, int64_t n, void *stream) {
    if (!x || !y) return se::train_fail(SE_ERR_ARG, "se_hifi_gate: null argument");
    unsigned nb;
    if (int rc = blocks_of("se_hifi_gate", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_gate, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, y, n);
    return launched("se_hifi_gate");
}

int se_hifi_skip(const float *yd, const float *uv, float *out, int S, int Co, int T, int Fy, int Fr, void *stream) {
    if (!yd || !uv || !out) return se::train_fail(SE_ERR_ARG, "se_hifi_skip: null argument");
    if (S <= 0 || Co <= 0 || T <= 0 || Fy <= 0 || Fr < Fy) return se::train_fail(SE_ERR_ARG, "se_hifi_skip: bad geometry (S %d, Co %d, T %d, Fy %d <= Fr %d)", S, Co, T, Fy, Fr);
    const long n = (long)S * Co * T * Fr;
    unsigned nb;
    if (int rc = blocks_of("se_hifi_skip", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_skip, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), yd, uv, out, n, Co, T, Fy, Fr);
    return launched("se_hifi_skip");
}

int se_hifi_rows(const float *x, float *rows, int Nc, int B, int C_, int T, int F, void *stream) {
    if (!x || !rows) return se::train_fail(SE_ERR_ARG, "se_hifi_rows: null argument");
    if (Nc <= 0 || B <= 0 || C_ <= 0 || T <= 0 || F <= 0) return se::train_fail(SE_ERR_ARG, "se_hifi_rows: bad geometry");
    const long n = (long)Nc * B * C_ * T * F;
    unsigned nb;
    if (int rc = blocks_of("se_hifi_rows", n, &nb)) return rc;
    hipLaunchKernelGGL(k_hifi_rows, dim3(nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, rows, n, Nc, B, C_, T, F);
    return launched("se_hifi_rows");
}

int se_hifi_lstm(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, int B, int TT, int H, void *stream) {
    return lstm_launch("se_hifi_lstm", gi, h0, c0, whh, out, hT, cT, nullptr, B, TT, H, stream);
}

int se_hifi_lstm_train_fwd(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, float *gates, float *cs, int B,
                           int TT, int H, void *stream) {
    if (!gates || !cs) return se::train_fail(SE_ERR_ARG, "se_hifi_lstm_train_fwd: null argument");
    return lstm_launch("se_hifi_lstm_train_fwd", gi, h0, c0, whh, out, hT, cT, nullptr, B, TT, H, stream, gates, cs);
}

int se_hifi_lstm_rows(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, const int *steps, int B, int TT, int H,
                      void *stream) {
    if (!steps) return se::train_fail(SE_ERR_ARG, "se_hifi_lstm_rows: null argument");
    return lstm_launch("se_hifi_lstm_rows", gi, h0, c0, whh, out, hT, cT, steps, B, TT, H, stream);
}

int se_hifi_lstm_train_fwd_rows(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, float *gates, float *cs,
                                const int *steps, int B, int TT, int H, void *stream) {
    if (!gates || !cs || !steps) return se::train_fail(SE_ERR_ARG, "se_hifi_lstm_train_fwd_rows: null argument");
    return lstm_launch("se_hifi_lstm_train_fwd_rows", gi, h0, c0, whh, out, hT, cT, steps, B, TT, H, stream, gates, cs);
}

int se_hifi_seqnorm(const float *o, const float *w, const float *bias, const float *mean_in, double step, float *wm, float *mean_out, float *y, int Nc, int B,
                    int C_, int T, int F, void *stream) {
    if (!o || !w || !bias || !mean_in || !wm || !mean_out || !y) return se::train_fail(SE_ERR_ARG, "se_hifi_seqnorm: null argument");
    if (Nc <= 0 || B <= 0 || (long)Nc * B > 65535 || C_ <= 0 || T <= 0 || F <= 0 || (long)T * C_ * F > (1L << 30) || step < 0.0)
        return se::train_fail(SE_ERR_ARG, "se_hifi_seqnorm: bad geometry (%d windows x %d utterances <= 65535, C %d, T %d, F %d, step %g)", Nc, B, C_, T, F, step);
    const int D = C_ * F, TD = T * D;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_hifi_winmean, dim3(Nc * B), dim3(kThreads), 0, st, o, wm, TD);
    hipLaunchKernelGGL(k_hifi_scan, dim3((B + 63) / 64), dim3(64), 0, st, wm, mean_in, mean_out, step, B, Nc, D);
    hipLaunchKernelGGL(k_hifi_normapply, dim3((TD + kThreads - 1) / kThreads, Nc * B), dim3(kThreads), 0, st, o, wm, w, bias, y, Nc, B, C_, T, F);
    return launched("se_hifi_seqnorm");
}

int se_hifi_seqnorm_rows(const float *o, const float *w, const float *bias, const float *mean_in, const int64_t *step, const int64_t *cnt, float *wm, float *mean_out,
                         float *y, int Nc, int B, int C_, int T, int F, void *stream) {
    if (!o || !w || !bias || !mean_in || !step || !cnt || !wm || !mean_out || !y) return se::train_fail(SE_ERR_ARG, "se_hifi_seqnorm_rows: null argument");
    if (Nc <= 0 || B <= 0 || (long)Nc * B > 65535 || C_ <= 0 || T <= 0 || F <= 0 || (long)T * C_ * F > (1L << 30))
        return se::train_fail(SE_ERR_ARG, "se_hifi_seqnorm_rows: bad geometry (%d windows x %d utterances <= 65535, C %d, T %d, F %d)", Nc, B, C_, T, F);
    const int D = C_ * F, TD = T * D;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_hifi_winmean, dim3(Nc * B), dim3(kThreads), 0, st, o, wm, TD);
    hipLaunchKernelGGL(k_hifi_scan_rows, dim3((B + 63) / 64), dim3(64), 0, st, wm, mean_in, mean_out, step, cnt, B, Nc, D);
    hipLaunchKernelGGL(k_hifi_normapply, dim3((TD + kThreads - 1) / kThreads, Nc * B), dim3(kThreads), 0, st, o, wm, w, bias, y, Nc, B, C_, T, F);
    return launched("se_hifi_seqnorm_rows");
}

}  // extern "C"
