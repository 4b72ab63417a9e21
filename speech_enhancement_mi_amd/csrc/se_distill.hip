// se_distill.hip - distillation training kernels behind se_distill_* and se_train_add_csum (include/se_engine.h).
//
// Feature loss of DistillationCRN (reference distillation_crn.py:549-572), for every map i of student s [S][Cs][X] and teacher
// t [S][Ct][X]:  u = W s (1x1 connector), v = BatchNorm2d(u), t' = max(t, margin_c), mask = 1 - (v <= t' & t' <= 0),
// loss_i = mean((v - t')^2 mask).  The work is memory-bound (the 1x1 contraction is at most 64 deep), so every pass streams the
// two maps once and recomputes u instead of storing it:
//   pass A  per (row, channel) partials of sum u, sum u^2 and the teacher's negative sum / count    -> fold A: mean, rstd, margin,
//                                                                                                     running statistics
//   pass B  per (row, channel) partials of the loss, sum dv and sum dv*xhat for a unit upstream     -> fold B: loss, channel sums
//   bwd     du = gamma rstd (dv - mean dv - xhat mean(dv xhat)); ds = W^T du; dW partial per row   -> fold W: dW, dgamma, dbeta
// One launch per pass covers all maps (grid.y = map, grid.x = row).  A workgroup owns one (map, row): thread (co, g) keeps the
// connector row W[co][:] in registers and accumulates its own channel over the columns x = g mod G of each staged tile, so the
// per-channel statistics need no atomics; the G partial sums and all row partials are folded in a fixed order (double), so the
// results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/se_engine.h"

namespace se {
int train_fail(int code, const char *fmt, ...);  // se_train.hip (owns se_train_last_error)
}

namespace {

constexpr int kMaxMaps = 8, kThreads = 256, kXT = 32, kMaxCs = 64, kMaxCt = 128;
constexpr float kBnEps = 1e-5f, kMomentum = 0.1f;
constexpr double kMarginEps = 1e-8;  // distillation_crn.py:12 EPS in get_margin

struct DMap {
    const float *s, *t, *w, *gamma, *beta;
    float *rm, *rv;
    int64_t *nbt;
    float *ds, *dw, *dgamma, *dbeta;
    int Cs, Ct;
    long X;
    int coff;     // channel offset of this map in the concatenated [sum Ct] per-channel arrays
    long woff;    // offset of this map's dW row partials (floats)
};

struct DArgs {
    DMap m[kMaxMaps];
    int nmaps, S, training, nch;   // nch = sum of Ct
    double *partA;   // [S][nch][4]  sum u, sum u^2, sum t<0, count t<0
    double *partB;   // [S][nch][3]  loss, sum dv, sum dv*xhat
    float *stat;     // [nch][4]     mean, rstd, margin
    double *csum;    // [nch][2]     sum dv, sum dv*xhat (unit upstream gradient)
    float *wpart;    // per map [S][Ct][Cs]
    float *loss;     // [1 + nmaps]
    const float *gout;
};

// MODE 0: pass A, 1: pass B, 2: backward
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_distill_pass(DArgs a) {
    __shared__ double sRed[kMaxCt * kMaxCs / 2];   // 32 KB: W (bwd), then the fixed-order reductions
    __shared__ float sS[kMaxCs][kXT + 1];
    __shared__ float sT[kMaxCt][kXT + 1];          // teacher tile; bwd: overwritten in place by du
    float *sW = reinterpret_cast<float *>(sRed);
    const DMap &m = a.m[blockIdx.y];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int Cs = m.Cs, Ct = m.Ct;
    const long X = m.X;
    const int G = kThreads / Ct, co = tid % Ct, g = tid / Ct;
    const bool active = g < G;
    const float *s = m.s + (long)row * Cs * X;
    const float *t = m.t + (long)row * Ct * X;

    float w[kMaxCs];
#pragma unroll
    for (int ci = 0; ci < kMaxCs; ci++) w[ci] = (active && ci < Cs) ? m.w[co * Cs + ci] : 0.f;
    float mean = 0.f, rstd = 0.f, margin = 0.f, gam = 0.f, bet = 0.f, mdv = 0.f, mdvx = 0.f, gg = 0.f;
    const double n_elem = (double)a.S * (double)X;
    const float scale = (float)(1.0 / ((double)a.S * Ct * (double)X * a.nmaps));   // d(total) / d(sum of squares of map i)
    if (MODE >= 1 && active) {
        const float *st = a.stat + 4 * (m.coff + co);
        mean = st[0]; rstd = st[1]; margin = st[2];
        gam = m.gamma[co]; bet = m.beta[co];
    }
    if (MODE == 2) {
        gg = a.gout[0];
        if (active && a.training) {
            mdv = (float)(a.csum[2 * (m.coff + co)] / n_elem);
            mdvx = (float)(a.csum[2 * (m.coff + co) + 1] / n_elem);
        }
        for (int i = tid; i < Ct * Cs; i += kThreads) sW[i] = m.w[i];
    }
    double acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    float dwa[kMaxCs];
#pragma unroll
    for (int ci = 0; ci < kMaxCs; ci++) dwa[ci] = 0.f;

    for (long x0 = 0; x0 < X; x0 += kXT) {
        const int nx = (int)(X - x0 < kXT ? X - x0 : kXT);
        __syncthreads();
        for (int i = tid; i < Cs * kXT; i += kThreads) {
            const int ci = i / kXT, xx = i % kXT;
            sS[ci][xx] = xx < nx ? s[(long)ci * X + x0 + xx] : 0.f;
        }
        for (int i = tid; i < Ct * kXT; i += kThreads) {
            const int c = i / kXT, xx = i % kXT;
            sT[c][xx] = xx < nx ? t[(long)c * X + x0 + xx] : 0.f;
        }
        __syncthreads();
        if (active) {
            for (int xx = g; xx < nx; xx += G) {
                float u = 0.f;
#pragma unroll
                for (int ci = 0; ci < kMaxCs; ci++)
                    if (ci < Cs) u = fmaf(w[ci], sS[ci][xx], u);
                const float tv = sT[co][xx];
                if (MODE == 0) {
                    acc0 += (double)u;
                    acc1 += (double)u * (double)u;
                    if (tv < 0.f) { acc2 += (double)tv; acc3 += 1.0; }
                } else {
                    const float xh = (u - mean) * rstd;
                    const float v = xh * gam + bet;
                    const float tp = fmaxf(tv, margin);
                    const float d = (v <= tp && tp <= 0.f) ? 0.f : v - tp;
                    const float dvu = 2.f * d * scale;
                    if (MODE == 1) {
                        acc0 += (double)d * (double)d;
                        acc1 += (double)dvu;
                        acc2 += (double)dvu * (double)xh;
                    } else {
                        const float du = a.training ? gg * gam * rstd * (dvu - mdv - xh * mdvx) : gg * gam * rstd * dvu;
                        sT[co][xx] = du;   // only this thread reads (co, xx)
#pragma unroll
                        for (int ci = 0; ci < kMaxCs; ci++)
                            if (ci < Cs) dwa[ci] = fmaf(du, sS[ci][xx], dwa[ci]);
                    }
                }
            }
        }
        if (MODE == 2 && m.ds) {
            __syncthreads();
            float *ds = m.ds + (long)row * Cs * X;
            for (int i = tid; i < Cs * kXT; i += kThreads) {
                const int ci = i / kXT, xx = i % kXT;
                if (xx < nx) {
                    float acc = 0.f;
                    for (int c = 0; c < Ct; c++) acc = fmaf(sW[c * Cs + ci], sT[c][xx], acc);
                    ds[(long)ci * X + x0 + xx] = acc;
                }
            }
        }
    }
    __syncthreads();
    if (MODE < 2) {
        constexpr int NV = MODE == 0 ? 4 : 3;
        if (active) {
            sRed[tid * NV + 0] = acc0; sRed[tid * NV + 1] = acc1; sRed[tid * NV + 2] = acc2;
            if (NV == 4) sRed[tid * NV + 3] = acc3;
        }
        __syncthreads();
        if (tid < Ct) {
            double r[NV];
            for (int k = 0; k < NV; k++) r[k] = 0;
            for (int q = 0; q < G; q++)
                for (int k = 0; k < NV; k++) r[k] += sRed[(q * Ct + tid) * NV + k];
            double *out = (MODE == 0 ? a.partA : a.partB) + ((long)row * a.nch + m.coff + tid) * NV;
            for (int k = 0; k < NV; k++) out[k] = r[k];
        }
    } else {
        for (int q = 0; q < G; q++) {   // fold the G column groups in a fixed order
            if (active && g == q) {
#pragma unroll
                for (int ci = 0; ci < kMaxCs; ci++)
                    if (ci < Cs) sW[co * Cs + ci] = (q == 0 ? 0.f : sW[co * Cs + ci]) + dwa[ci];
            }
            __syncthreads();
        }
        float *wp = a.wpart + m.woff + (long)row * Ct * Cs;
        for (int i = tid; i < Ct * Cs; i += kThreads) wp[i] = sW[i];
    }
}

__device__ inline int map_of(const DArgs &a, int ch) {
    int k = 0;
    while (k + 1 < a.nmaps && ch >= a.m[k + 1].coff) k++;
    return k;
}

// one thread per (map, channel): fold the row partials of pass A, set the normalisation and update the running statistics
__global__ __launch_bounds__(1024) void k_distill_fold_a(DArgs a) {
    const int ch = threadIdx.x;
    if (ch >= a.nch) return;
    const DMap &m = a.m[map_of(a, ch)];
    const int co = ch - m.coff;
    double su = 0, suu = 0, tn = 0, cn = 0;
    for (int r = 0; r < a.S; r++) {
        const double *p = a.partA + ((long)r * a.nch + ch) * 4;
        su += p[0]; suu += p[1]; tn += p[2]; cn += p[3];
    }
    const double n = (double)a.S * (double)m.X;
    float mean, rstd;
    if (a.training) {
        const double mu = su / n;
        double var = suu / n - mu * mu;
        var = var > 0 ? var : 0;
        mean = (float)mu;
        rstd = 1.f / sqrtf((float)var + kBnEps);
        if (m.rm) m.rm[co] = (1.f - kMomentum) * m.rm[co] + kMomentum * mean;
        if (m.rv) m.rv[co] = (1.f - kMomentum) * m.rv[co] + kMomentum * (float)(n > 1 ? var * n / (n - 1) : var);
        if (co == 0 && m.nbt) m.nbt[0] += 1;
    } else {
        mean = m.rm[co];
        rstd = 1.f / sqrtf(m.rv[co] + kBnEps);
    }
    float *st = a.stat + 4 * ch;
    st[0] = mean; st[1] = rstd; st[2] = (float)(tn / (cn + kMarginEps)); st[3] = 0.f;
}

// one thread per (map, channel): fold pass B; thread 0 then folds the channels of every map in order into the loss
__global__ __launch_bounds__(1024) void k_distill_fold_b(DArgs a) {
    __shared__ double sl[kMaxMaps * kMaxCt];
    const int ch = threadIdx.x;
    if (ch < a.nch) {
        double l = 0, dv = 0, dvx = 0;
        for (int r = 0; r < a.S; r++) {
            const double *p = a.partB + ((long)r * a.nch + ch) * 3;
            l += p[0]; dv += p[1]; dvx += p[2];
        }
        sl[ch] = l;
        a.csum[2 * ch] = dv;
        a.csum[2 * ch + 1] = dvx;
    }
    __syncthreads();
    if (ch == 0) {
        double total = 0;
        for (int k = 0; k < a.nmaps; k++) {
            const DMap &m = a.m[k];
            double l = 0;
            for (int c = 0; c < m.Ct; c++) l += sl[m.coff + c];
            const double lk = l / ((double)a.S * m.Ct * (double)m.X);
            a.loss[1 + k] = (float)lk;
            total += lk;
        }
        a.loss[0] = (float)(total / a.nmaps);
    }
}

// one thread per dW entry of every map: fold the row partials; the ci == 0 threads also write dgamma / dbeta
__global__ __launch_bounds__(256) void k_distill_fold_w(DArgs a, long total) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int k = 0;
    while (k + 1 < a.nmaps && e >= a.m[k + 1].woff / a.S) k++;
    const DMap &m = a.m[k];
    const long local = e - m.woff / a.S, per = (long)m.Ct * m.Cs;
    double acc = 0;
    for (int r = 0; r < a.S; r++) acc += (double)a.wpart[m.woff + (long)r * per + local];
    m.dw[local] = (float)acc;
    if (local % m.Cs == 0) {
        const int co = (int)(local / m.Cs);
        const float gg = a.gout[0];
        m.dgamma[co] = gg * (float)a.csum[2 * (m.coff + co) + 1];
        m.dbeta[co] = gg * (float)a.csum[2 * (m.coff + co)];
    }
}

// dst[s][c][:] += src[s][c][:]; part[s][c] = sum of the result (one workgroup per (s, c), fixed reduction order)
__global__ __launch_bounds__(256) void k_add_csum(float *dst, const float *src, float *part, long X) {
    __shared__ float red[4];
    const long base = ((long)blockIdx.y * gridDim.x + blockIdx.x) * X;
    float acc = 0.f;
    for (long x = threadIdx.x; x < X; x += 256) {
        const float v = dst[base + x] + src[base + x];
        dst[base + x] = v;
        acc += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct WsLayout {
    size_t partA, partB, stat, csum, wpart, total;
};

int plan(const se_distill_map *maps, int nmaps, int S, DArgs &a, WsLayout &L) {
    if (!maps || nmaps < 1 || nmaps > kMaxMaps || S < 1) return se::train_fail(SE_ERR_ARG, "se_distill: nmaps %d (1..%d), S %d", nmaps, kMaxMaps, S);
    a = DArgs{};
    a.nmaps = nmaps;
    a.S = S;
    int nch = 0;
    long wfl = 0;
    for (int k = 0; k < nmaps; k++) {
        const se_distill_map &q = maps[k];
        if (q.Cs < 1 || q.Cs > kMaxCs || q.Ct < 1 || q.Ct > kMaxCt || q.X < 1)
            return se::train_fail(SE_ERR_ARG, "se_distill: map %d has Cs %d (1..%d), Ct %d (1..%d), X %d", k, q.Cs, kMaxCs, q.Ct, kMaxCt, q.X);
        DMap &m = a.m[k];
        m.s = q.s; m.t = q.t; m.w = q.w; m.gamma = q.gamma; m.beta = q.beta; m.rm = q.running_mean; m.rv = q.running_var;
        m.nbt = q.num_batches_tracked; m.ds = q.ds; m.dw = q.dw; m.dgamma = q.dgamma; m.dbeta = q.dbeta;
        m.Cs = q.Cs; m.Ct = q.Ct; m.X = q.X; m.coff = nch; m.woff = wfl;
        nch += q.Ct;
        wfl += (long)S * q.Ct * q.Cs;
    }
    a.nch = nch;
    L.partA = 0;
    L.partB = L.partA + align256(sizeof(double) * 4 * (size_t)S * nch);
    L.stat = L.partB + align256(sizeof(double) * 3 * (size_t)S * nch);
    L.csum = L.stat + align256(sizeof(float) * 4 * (size_t)nch);
    L.wpart = L.csum + align256(sizeof(double) * 2 * (size_t)nch);
    L.total = L.wpart + align256(sizeof(float) * (size_t)wfl);
    return SE_OK;
}

void bind(DArgs &a, const WsLayout &L, void *ws) {
    char *b = static_cast<char *>(ws);
    a.partA = reinterpret_cast<double *>(b + L.partA);
    a.partB = reinterpret_cast<double *>(b + L.partB);
    a.stat = reinterpret_cast<float *>(b + L.stat);
    a.csum = reinterpret_cast<double *>(b + L.csum);
    a.wpart = reinterpret_cast<float *>(b + L.wpart);
}

}  // namespace

extern "C" {

int se_train_add_csum(float *dst, const float *src, float *part, int S, int C, int64_t X, void *stream) {
    if (!dst || !src || !part || S < 1 || C < 1 || X < 1) return se::train_fail(SE_ERR_ARG, "se_train_add_csum: bad argument");
    hipLaunchKernelGGL(k_add_csum, dim3(C, S), dim3(256), 0, static_cast<hipStream_t>(stream), dst, src, part, (long)X);
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "se_train_add_csum launch failed");
}

int64_t se_distill_ws_bytes(const se_distill_map *maps, int nmaps, int S) {
    DArgs a;
    WsLayout L;
    const int rc = plan(maps, nmaps, S, a, L);
    return rc != SE_OK ? rc : (int64_t)L.total;
}

int se_distill_fwd(const se_distill_map *maps, int nmaps, int S, int training, void *ws, float *loss, void *stream) {
    DArgs a;
    WsLayout L;
    int rc = plan(maps, nmaps, S, a, L);
    if (rc != SE_OK) return rc;
    if (!ws || !loss) return se::train_fail(SE_ERR_ARG, "se_distill_fwd: null workspace / loss");
    for (int k = 0; k < nmaps; k++) {
        const DMap &m = a.m[k];
        if (!m.s || !m.t || !m.w || !m.gamma || !m.beta || !m.rm || !m.rv) return se::train_fail(SE_ERR_ARG, "se_distill_fwd: map %d has a null input", k);
    }
    bind(a, L, ws);
    a.training = training != 0;
    a.loss = loss;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_distill_pass<0>, dim3(S, nmaps), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_distill_fold_a, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(k_distill_pass<1>, dim3(S, nmaps), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_distill_fold_b, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "se_distill_fwd launch failed");
}

int se_distill_bwd(const se_distill_map *maps, int nmaps, int S, int training, void *ws, const float *gout, void *stream) {
    DArgs a;
    WsLayout L;
    int rc = plan(maps, nmaps, S, a, L);
    if (rc != SE_OK) return rc;
    if (!ws || !gout) return se::train_fail(SE_ERR_ARG, "se_distill_bwd: null workspace / upstream gradient");
    long total = 0;
    for (int k = 0; k < nmaps; k++) {
        const DMap &m = a.m[k];
        if (!m.s || !m.t || !m.w || !m.gamma || !m.beta || !m.dw || !m.dgamma || !m.dbeta)
            return se::train_fail(SE_ERR_ARG, "se_distill_bwd: map %d has a null input / gradient", k);
        total += (long)m.Ct * m.Cs;
    }
    bind(a, L, ws);
    a.training = training != 0;
    a.gout = gout;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_distill_pass<2>, dim3(S, nmaps), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_distill_fold_w, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    return hipGetLastError() == hipSuccess ? SE_OK : se::train_fail(SE_ERR_HIP, "se_distill_bwd launch failed");
}

}  // extern "C"
