// se_pesq.hip - the perceptual term of GTSA.compute_loss as hand-written kernels, forward and backward (se_loss_pesq_* C ABI).
//
// Reference: utility.pesq_loss utility.py:615-814 on torchaudio's Spectrogram(1024, 512, 256, power=2); restated in losses._pesq_d as
// batched torch code whose time recurrence is a Python loop over the frames (about 190 steps for 3 s, forward and backward).  Here the
// same arithmetic is 2 launches forward and 3 backward:
//
//   k_pesq_spec       grid (frame, row, signal): 512 Hann-weighted samples gathered through the reflect rule of the row's OWN end, the
//                     1024-point real transform as one 512-point complex Stockham transform (fft_lds.h, 4*4*4*4*2) + rfft_post,
//                     |X|^2 summed into 49 raw Bark-band sums and the frame's level partial over bins [19, 192); the predicted
//                     signal's complex spectrum is kept for the backward
//   k_pesq_row_fwd    one workgroup per row, everything from level alignment to the scalar: fixed-order level and band-mean
//                     reductions, masks, band equalisation, the 2-term time recurrence (serial, one thread), loudness, both
//                     disturbances per frame, syllable and tail aggregation.  Saves per frame: the silence bit, both totals, s_t,
//                     sym and asym before the cap; per band: the equalisation factor (clamped and not) and the clean mean; the levels.
//   k_pesq_row_bwd    the scalar back to d loss / d (raw predicted band sum)[49][T] and d loss / d (predicted level): every
//                     data-dependent branch is re-taken from the saved values, the recurrence's adjoint g_t += 0.2 g_{t+1} through
//                     its clamp is the one serial pass
//   k_pesq_spec_bwd   per frame: dX = 2 X dP, the adjoint of the real transform (irfft_pre + the same Stockham passes) and the window
//   k_pesq_gather_bwd every sample gathers its <= 2 frames plus its mirror terms from the reflect padding
//
// The row kernels compute in double (a few hundred thousand operations per row; the spectra stay float): what separates the kernels
// from a float64 evaluation is then the float transform alone.  No atomics anywhere; every reduction runs in a fixed order, so a row's
// value and gradient are bit-reproducible and do not depend on the other rows of the batch.  A row with fewer than 20 frames
// (lens[b] < 4864) is a bounded branch: NaN value, zero gradient, nothing of it is read.
// PARITY: pinned by tests/golden/pesq_golden.npz (unpinned at the torchaudio boundary, see losses.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>

#include "../../include/se_engine.h"
#include "fft_lds.h"

namespace {

constexpr int kNB = 49, kBins = 513, kHop = 256, kWin = 512, kN2 = 512;
constexpr int kLowF = 19, kHighF = 192;     // int(2 * 300 / 16000 * 513), int(2 * 3000 / 16000 * 513), utility.py:731-732
constexpr int kMinLen = 4864;               // 20 frames
constexpr int kMaxT = 896;                  // frames a row kernel holds in LDS (8 doubles each): 14.3 s
constexpr double kSl = 1.866055e-1;         // utility.py:654
constexpr int kFr = 6;                      // per-frame saves: ns, tt, tp, s, sym / h, asym / h
typedef double real;

struct PesqShape {
    int B;
    long L;
    int Tm, NBm;
    long Rt, Rp, gBp, gBt, lvT, lvP, fr, bd, sc, Xp, dfr, total;  // workspace offsets in floats
};

__host__ __device__ inline PesqShape pesq_shape(int B, long L) {
    PesqShape s{};
    s.B = B; s.L = L;
    s.Tm = (int)(1 + L / kHop);
    s.NBm = (s.Tm - 20) / 10 + 1;
    long o = 0;
    auto take = [&](long n) { const long at = o; o += (n + 3) & ~3L; return at; };
    const long bt = (long)B * kNB * s.Tm;
    s.Rt = take(bt); s.Rp = take(bt); s.gBp = take(bt); s.gBt = take(bt);
    s.lvT = take((long)B * s.Tm); s.lvP = take((long)B * s.Tm);
    s.fr = take((long)B * kFr * s.Tm * 2);  // doubles
    s.bd = take((long)B * 3 * 64 * 2);      // doubles: e, e before the clamp, clean band mean
    s.sc = take((long)B * 8 * 2);           // doubles: gain true, gain pred, sres, asres, d loss / d (pred level sum)
    s.Xp = take((long)B * s.Tm * kBins * 2);
    s.dfr = take((long)B * s.Tm * kWin);
    s.total = o;
    return s;
}

struct RowGeo {
    long len;
    int T, nb, left;
    bool ok;
};

__device__ inline RowGeo row_geo(const int64_t *lens, int b, long L) {
    RowGeo g;
    const long v = lens[b];
    g.len = v < 0 ? 0 : (v > L ? L : v);
    g.ok = g.len >= kMinLen;
    g.T = (int)(1 + g.len / kHop);
    g.nb = g.ok ? (g.T - 20) / 10 + 1 : 1;
    g.left = g.T - 10 * g.nb;
    return g;
}

// grid (Tm, B, 2), 256 threads.  z = 0: clean -> Rt, lvT; z = 1: prediction -> Rp, lvP, Xp
__global__ __launch_bounds__(256) void k_pesq_spec(const float *clean, const float *pred, const int64_t *lens, long L, int Tm, const float *win,
                                                   const int *edges, float *Rt, float *Rp, float *lvT, float *lvP, float *Xp) {
    __shared__ cf2 za[kN2], zb[kN2], tw[2 * kN2];
    __shared__ float pw[kBins + 3];
    const int t = blockIdx.x, b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x;
    const RowGeo g = row_geo(lens, b, L);
    float *R = (sig ? Rp : Rt) + (long)b * kNB * Tm, *lv = (sig ? lvP : lvT) + (long)b * Tm;
    if (!g.ok || t >= g.T) {  // beyond the row's frames: zeros, nothing of the row is read
        if (tid < kNB) R[(long)tid * Tm + t] = 0.0f;
        if (tid == 64) lv[t] = 0.0f;
        return;
    }
    const float *x = (sig ? pred : clean) + (long)b * L;
    for (int i = tid; i < 2 * kN2; i += 256) {
        float sn, cs;
        sincospif(-(float)i / (float)kN2, &sn, &cs);  // exp(-2 pi i m / 1024)
        tw[i] = cf2{cs, sn};
    }
    for (int n = tid; n < kN2; n += 256) {  // z[n] = frame[2n] + i frame[2n + 1]; the window covers frame positions [256, 768)
        float v[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int q = 2 * n + h;
            float s = 0.0f;
            if (q >= 256 && q < 768) {
                long m = (long)t * kHop - 512 + q;
                m = m < 0 ? -m : m;
                if (m >= g.len) m = 2 * (g.len - 1) - m;
                m = m < 0 ? 0 : (m > g.len - 1 ? g.len - 1 : m);
                s = win[q - 256] * x[m];
            }
            v[h] = s;
        }
        za[n] = cf2{v[0], v[1]};
    }
    __syncthreads();
    fft_pass<4>(za, zb, kN2, kN2, 1, 1, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(zb, za, kN2, kN2, 1, 4, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(za, zb, kN2, kN2, 1, 16, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(zb, za, kN2, kN2, 1, 64, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<2>(za, zb, kN2, kN2, 1, 256, tw, tid, 256, 2);
    __syncthreads();
    float *xp = sig ? Xp + ((long)b * Tm + t) * kBins * 2 : nullptr;
    for (int k = tid; k < kBins; k += 256) {
        const cf2 X = rfft_post(zb, k, kN2, tw);
        pw[k] = X.x * X.x + X.y * X.y;
        if (xp) { xp[2 * k] = X.x; xp[2 * k + 1] = X.y; }
    }
    __syncthreads();
    if (tid < kNB) {
        float s = 0.0f;
        for (int k = edges[tid]; k < edges[tid + 1]; k++) s += pw[k];
        R[(long)tid * Tm + t] = s;
    } else if (tid >= 64 && tid < 128) {  // the frame's level partial: bins [19, 192) in a fixed order
        const int lane = tid - 64;
        float s = 0.0f;
        for (int k = kLowF + lane; k < kHighF; k += 64) s += pw[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) lv[t] = s;
    }
}

// ---- row kernels ---------------------------------------------------------------------------------------------------------------------
struct BandC {
    real c, thr, zp, k2, w;
};
__device__ inline BandC band_c(const real *tab, int j) { return BandC{tab[j], tab[kNB + j], tab[2 * kNB + j], tab[3 * kNB + j], tab[4 * kNB + j]}; }
__device__ inline real zw_base(real Bv, const BandC &k) { return 0.5 + 0.5 * Bv / k.thr; }
__device__ inline real loud(real Bv, const BandC &k) { return k.k2 * (pow(zw_base(Bv, k), k.zp) - 1.0) * kSl; }
__device__ inline real dloud(real Bv, const BandC &k) { return k.k2 * kSl * k.zp * pow(zw_base(Bv, k), k.zp - 1.0) * 0.5 / k.thr; }
__device__ inline real clampr(real v, real lo, real hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline real wave_sum(real v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ inline real block_sum(real v, real *red) {  // 256 threads, fixed order; every thread gets the sum
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// f_k = power-6 mean of block k (20 frames every 10; k == nb: the last `left` frames) + 1e-8 of the capped per-frame values
__device__ inline real block_f(const real *X, int k, const RowGeo &g) {
    const int t0 = k < g.nb ? 10 * k : g.T - g.left, n = k < g.nb ? 20 : g.left;
    real s = 0;
    for (int i = 0; i < n; i++) {
        const real v = X[t0 + i] > 45.0 ? 45.0 : X[t0 + i];
        const real v2 = v * v;
        s += v2 * v2 * v2;
    }
    return s / (real)n + 1e-8;
}

// per-(band, frame) forward values the backward re-derives too
struct Cell {
    real Bp, Bt, Lp, Lt, d, m, D, h0, h, ratio;
    bool mp, mt;
};
__device__ inline Cell cell(real rp, real rt, real gp, real gt, real e, real c, const BandC &k) {
    Cell x;
    x.Bp = rp * gp * k.c;
    x.Bt = rt * gt * k.c * e;
    x.mp = x.Bp > k.thr;
    x.mt = x.Bt > k.thr;
    x.Lp = x.mp ? loud(x.Bp * c, k) : 0.0;
    x.Lt = x.mt ? loud(x.Bt, k) : 0.0;
    x.d = x.Lp - x.Lt;
    x.m = 0.25 * (x.Lp < x.Lt ? x.Lp : x.Lt);
    x.D = x.d > x.m ? x.d - x.m : (x.d < -x.m ? x.d + x.m : 0.0);
    x.ratio = (x.Lp + 50.0) / (x.Lt + 50.0);
    x.h0 = pow(x.ratio, 1.2);
    x.h = x.h0 < 3.0 ? 0.0 : (x.h0 > 12.0 ? 12.0 : x.h0);
    return x;
}

// LDS of a row kernel: 8 per-frame arrays of Tm doubles, then [5][49] band constants, 4 x 64 band values, NBm + 1 block values twice, 4 partials
__device__ inline void row_lds(real *sh, int Tm, int NBm, real *(&fr)[8], real *&tab, real *&bv, real *&blk, real *&red) {
    for (int i = 0; i < 8; i++) fr[i] = sh + (long)i * Tm;
    tab = sh + 8L * Tm;
    bv = tab + 5 * kNB + 3;
    blk = bv + 4 * 64;
    red = blk + 2 * (NBm + 1);
}
inline size_t row_lds_bytes(int Tm, int NBm) { return sizeof(real) * (8L * Tm + 5 * kNB + 3 + 4 * 64 + 2 * (NBm + 1) + 4); }

__global__ __launch_bounds__(256) void k_pesq_row_fwd(const float *Rt, const float *Rp, const float *lvT, const float *lvP, const int64_t *lens, long L, int Tm, int NBm,
                                                      const float *band_tab, real *fr_out, real *bd_out, real *sc_out, float *val) {
    extern __shared__ __align__(16) unsigned char sh_raw[];
    real *fr[8], *tab, *bv, *blk, *red;
    row_lds(reinterpret_cast<real *>(sh_raw), Tm, NBm, fr, tab, bv, blk, red);
    real *ns = fr[0], *tts = fr[1], *tps = fr[2], *ss = fr[3], *Ss = fr[4], *As = fr[5];
    real *e = bv, *eraw = bv + 64, *at = bv + 128;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RowGeo g = row_geo(lens, b, L);
    if (!g.ok) {  // the whole workgroup leaves: no value for fewer than 20 frames
        if (tid == 0) val[b] = NAN;
        return;
    }
    const int T = g.T;
    for (int i = tid; i < 5 * kNB; i += 256) tab[i] = (real)band_tab[i];
    const float *rt = Rt + (long)b * kNB * Tm, *rp = Rp + (long)b * kNB * Tm;
    real a = 0, p = 0;
    for (int t = tid; t < T; t += 256) { a += (real)lvT[(long)b * Tm + t]; p += (real)lvP[(long)b * Tm + t]; }
    const real nlev = (real)(kHighF - kLowF) * (real)T;
    const real gt = 1e7 / (block_sum(a, red) / nlev + 1e-14), gp = 1e7 / (block_sum(p, red) / nlev + 1e-14);
    real W = 0;
    for (int j = 0; j < kNB; j++) W += tab[4 * kNB + j];
    // silence bit from the un-equalised clean totals
    for (int t = tid; t < T; t += 256) {
        real tt0 = 0;
        for (int j = 0; j < kNB; j++) {
            const real v = (real)rt[(long)j * Tm + t] * gt * tab[j];
            if (v > tab[kNB + j]) tt0 += v;
        }
        ns[t] = tt0 > 1e7 ? 1.0 : 0.0;
    }
    __syncthreads();
    // band equalisation: the ratio of the time means over the non-silent frames, one wave per band
    for (int j = wave; j < kNB; j += 4) {
        real sa = 0, sp = 0;
        for (int t = lane; t < T; t += 64) {
            if (ns[t] != 0.0) {
                const real vt = (real)rt[(long)j * Tm + t] * gt * tab[j], vp = (real)rp[(long)j * Tm + t] * gp * tab[j];
                if (vt > tab[kNB + j]) sa += vt;
                if (vp > tab[kNB + j]) sp += vp;
            }
        }
        sa = wave_sum(sa);
        sp = wave_sum(sp);
        if (lane == 0) {
            at[j] = sa / (real)T;
            eraw[j] = (sp / (real)T + 1e3) / (at[j] + 1e3);
            e[j] = clampr(eraw[j], 0.01, 100.0);
        }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        real tt = 0, tp = 0;
        for (int j = 0; j < kNB; j++) {
            const real vt = (real)rt[(long)j * Tm + t] * gt * tab[j] * e[j], vp = (real)rp[(long)j * Tm + t] * gp * tab[j];
            if (vt > tab[kNB + j]) tt += vt;
            if (vp > tab[kNB + j]) tp += vp;
        }
        tts[t] = tt;
        tps[t] = tp;
    }
    __syncthreads();
    if (tid == 0) {  // s_t = 0.2 s_{t-1} + (total_true_t + 5e3) / (total_pred_t + 5e3), s_{-1} = 1
        real s = 1.0;
        for (int t = 0; t < T; t++) { s = 0.2 * s + (tts[t] + 5e3) / (tps[t] + 5e3); ss[t] = s; }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const real c = clampr(ss[t], 3e-4, 5.0);
        real Q = 0, A = 0;
        for (int j = 0; j < kNB; j++) {
            const BandC k = band_c(tab, j);
            const Cell x = cell((real)rp[(long)j * Tm + t], (real)rt[(long)j * Tm + t], gp, gt, e[j], c, k);
            const real dw = fabs(x.D) * k.w;
            Q += dw * dw;
            A += fabs(x.D * x.h) * k.w;
        }
        const real hh = pow((tts[t] + 1e5) / 1e7, 0.04);
        Ss[t] = sqrt(Q / W) * W / hh;
        As[t] = A / W * W / hh;
    }
    __syncthreads();
    for (int k = tid; k <= g.nb; k += 256) { blk[k] = block_f(Ss, k, g); blk[NBm + 1 + k] = block_f(As, k, g); }
    __syncthreads();
    if (tid == 0) {
        real qs = 0, qa = 0;
        for (int k = 0; k <= g.nb; k++) { qs += cbrt(blk[k]); qa += cbrt(blk[NBm + 1 + k]); }  // (f ** (1 / 6)) ** 2
        const real sres = sqrt(qs / (real)(g.nb + 1) + 1e-8), asres = sqrt(qa / (real)(g.nb + 1) + 1e-8);
        val[b] = (float)-(4.5 - 0.1 * sres - 0.0309 * asres);
        real *sc = sc_out + (long)b * 8;
        sc[0] = gt; sc[1] = gp; sc[2] = sres; sc[3] = asres;
    }
    for (int i = 0; i < kFr; i++)
        for (int t = tid; t < T; t += 256) fr_out[((long)b * kFr + i) * Tm + t] = fr[i][t];
    if (tid < kNB) {
        bd_out[((long)b * 3 + 0) * 64 + tid] = e[tid];
        bd_out[((long)b * 3 + 1) * 64 + tid] = eraw[tid];
        bd_out[((long)b * 3 + 2) * 64 + tid] = at[tid];
    }
}

// gBp leaves as d loss / d (raw predicted band sum), sc[4] as d loss / d (sum of the predicted level partials)
__global__ __launch_bounds__(256) void k_pesq_row_bwd(const float *Rt, const float *Rp, const int64_t *lens, long L, int Tm, int NBm, const float *band_tab,
                                                      const real *fr_in, const real *bd_in, real *sc_io, const float *gV, float *gBp, float *gBt) {
    extern __shared__ __align__(16) unsigned char sh_raw[];
    real *fr[8], *tab, *bv, *blk, *red;
    row_lds(reinterpret_cast<real *>(sh_raw), Tm, NBm, fr, tab, bv, blk, red);
    real *ns = fr[0], *tts = fr[1], *tps = fr[2], *ss = fr[3], *Ss = fr[4], *As = fr[5], *gs = fr[6], *aux = fr[7];
    real *e = bv, *eraw = bv + 64, *at = bv + 128, *dap = bv + 192;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RowGeo g = row_geo(lens, b, L);
    if (!g.ok) return;  // k_pesq_gather_bwd writes this row's zeros
    const int T = g.T;
    for (int i = tid; i < 5 * kNB; i += 256) tab[i] = (real)band_tab[i];
    for (int i = 0; i < kFr; i++)
        for (int t = tid; t < T; t += 256) fr[i][t] = fr_in[((long)b * kFr + i) * Tm + t];
    if (tid < kNB) {
        e[tid] = bd_in[((long)b * 3 + 0) * 64 + tid];
        eraw[tid] = bd_in[((long)b * 3 + 1) * 64 + tid];
        at[tid] = bd_in[((long)b * 3 + 2) * 64 + tid];
    }
    real *sc = sc_io + (long)b * 8;
    const real gt = sc[0], gp = sc[1], sres = sc[2], asres = sc[3], gl = (real)gV[b];
    const float *rt = Rt + (long)b * kNB * Tm, *rp = Rp + (long)b * kNB * Tm;
    float *gbp = gBp + (long)b * kNB * Tm, *gbt = gBt + (long)b * kNB * Tm;
    __syncthreads();
    real W = 0;
    for (int j = 0; j < kNB; j++) W += tab[4 * kNB + j];
    // d loss / d f_k of every block: loss = -4.5 + 0.1 sres + 0.0309 asres, res = sqrt(mean_k f_k ** (1 / 3) + 1e-8)
    for (int k = tid; k <= g.nb; k += 256) {
        const real fs = block_f(Ss, k, g), fa = block_f(As, k, g);
        blk[k] = 0.1 * gl * 0.5 / sres / (real)(g.nb + 1) / (3.0 * cbrt(fs * fs));
        blk[NBm + 1 + k] = 0.0309 * gl * 0.5 / asres / (real)(g.nb + 1) / (3.0 * cbrt(fa * fa));
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        real gS = 0, gA = 0;  // d loss / d (sym / h), d loss / d (asym / h): zero above the cap at 45
        const int k1 = t / 10;
        for (int which = 0; which < 2; which++) {
            const real v = which ? As[t] : Ss[t];
            const real *df = blk + which * (NBm + 1);
            real gacc = 0;
            if (v <= 45.0) {
                const real v5 = 6.0 * v * v * v * v * v;
                if (k1 < g.nb) gacc += df[k1] / 20.0 * v5;
                if (k1 >= 1 && k1 - 1 < g.nb) gacc += df[k1 - 1] / 20.0 * v5;
                if (t >= T - g.left) gacc += df[g.nb] / (real)g.left * v5;
            }
            if (which) gA = gacc; else gS = gacc;
        }
        const real tt = tts[t];
        const real hh = pow((tt + 1e5) / 1e7, 0.04);
        const real dsym = gS / hh, dasym = gA / hh;
        const real dtt_h = -(gS * Ss[t] + gA * As[t]) * 0.04 / (tt + 1e5);
        const real sym = Ss[t] * hh;
        const real dQ = sym > 0.0 ? dsym * 0.5 * W / sym : 0.0;  // sym = sqrt(Q / W) W; a frame of zero disturbance gets a zero gradient
        const real c = clampr(ss[t], 3e-4, 5.0);
        real dc = 0;
        for (int j = 0; j < kNB; j++) {
            const BandC k = band_c(tab, j);
            const Cell x = cell((real)rp[(long)j * Tm + t], (real)rt[(long)j * Tm + t], gp, gt, e[j], c, k);
            const real Ah = x.D * x.h, sg = Ah > 0.0 ? 1.0 : (Ah < 0.0 ? -1.0 : 0.0);
            const real dD = dQ * 2.0 * x.D * k.w * k.w + dasym * k.w * sg * x.h, dh = dasym * k.w * sg * x.D;
            real dLp = 0, dLt = 0, dm = 0;
            if (x.h0 >= 3.0 && x.h0 <= 12.0) {
                const real dr = dh * 1.2 * x.h0 / x.ratio;
                dLp += dr / (x.Lt + 50.0);
                dLt -= dr * x.ratio / (x.Lt + 50.0);
            }
            if (x.d > x.m) { dLp += dD; dLt -= dD; dm = -dD; }
            else if (x.d < -x.m) { dLp += dD; dLt -= dD; dm = dD; }
            if (x.Lp < x.Lt) dLp += 0.25 * dm; else dLt += 0.25 * dm;
            const real dBp2 = x.mp ? dLp * dloud(x.Bp * c, k) : 0.0;
            const real dBt = x.mt ? dLt * dloud(x.Bt, k) : 0.0;
            dc += dBp2 * x.Bp;
            gbp[(long)j * Tm + t] = (float)(dBp2 * c);
            gbt[(long)j * Tm + t] = (float)dBt;
        }
        gs[t] = (ss[t] >= 3e-4 && ss[t] <= 5.0) ? dc : 0.0;
        aux[t] = dtt_h;
    }
    __syncthreads();
    if (tid == 0) {  // adjoint of the recurrence: g_t += 0.2 g_{t+1}
        real acc = 0;
        for (int t = T - 1; t >= 0; t--) { acc = gs[t] + 0.2 * acc; gs[t] = acc; }
    }
    __syncthreads();
    for (int t = tid; t < T; t += 256) {
        const real den = tps[t] + 5e3, r = (tts[t] + 5e3) / den;
        const real dtt = aux[t] + gs[t] / den, dtp = -gs[t] * r / den;
        for (int j = 0; j < kNB; j++) {
            const real vt = (real)rt[(long)j * Tm + t] * gt * tab[j] * e[j], vp = (real)rp[(long)j * Tm + t] * gp * tab[j];
            if (vt > tab[kNB + j]) gbt[(long)j * Tm + t] += (float)dtt;
            if (vp > tab[kNB + j]) gbp[(long)j * Tm + t] += (float)dtp;
        }
    }
    __syncthreads();
    for (int j = wave; j < kNB; j += 4) {  // through the equalisation factor into the predicted band mean
        real de = 0;
        for (int t = lane; t < T; t += 64) de += (real)gbt[(long)j * Tm + t] * ((real)rt[(long)j * Tm + t] * gt * tab[j]);
        de = wave_sum(de);
        if (lane == 0) dap[j] = (eraw[j] >= 0.01 && eraw[j] <= 100.0) ? de / (at[j] + 1e3) : 0.0;
    }
    __syncthreads();
    real part = 0;
    for (int t = tid; t < T; t += 256) {
        real acc = 0;
        for (int j = 0; j < kNB; j++) {
            const real raw = (real)rp[(long)j * Tm + t], vp = raw * gp * tab[j];
            real gb = (real)gbp[(long)j * Tm + t];
            if (vp > tab[kNB + j] && ns[t] != 0.0) gb += dap[j] / (real)T;
            gbp[(long)j * Tm + t] = (float)(gb * gp * tab[j]);
            acc += gb * raw * tab[j];
        }
        part += acc;
    }
    const real dgp = block_sum(part, red);
    if (tid == 0) sc[4] = -dgp * gp * gp / 1e7 / ((real)(kHighF - kLowF) * (real)T);  // gain = 1e7 / (sum / (173 T) + 1e-14)
}

// grid (Tm, B): dfr[b][t][j] = Hann[j] * d loss / d (windowed sample j of frame t)
__global__ __launch_bounds__(256) void k_pesq_spec_bwd(const float *Xp, const float *gBp, const real *sc_in, const int64_t *lens, long L, int Tm, const float *win,
                                                       const int *band_of, float *dfr) {
    __shared__ cf2 za[kN2], zb[kN2], tw[2 * kN2], Y[kBins + 1];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const RowGeo g = row_geo(lens, b, L);
    if (!g.ok || t >= g.T) return;  // k_pesq_gather_bwd never reads these frames
    for (int i = tid; i < 2 * kN2; i += 256) {
        float sn, cs;
        sincospif(-(float)i / (float)kN2, &sn, &cs);
        tw[i] = cf2{cs, sn};
    }
    const float *xp = Xp + ((long)b * Tm + t) * kBins * 2, *gb = gBp + (long)b * kNB * Tm;
    const float dE = (float)sc_in[(long)b * 8 + 4];
    for (int k = tid; k < kBins; k += 256) {  // G = dRe + i dIm = 2 X dP; the sum over k of Re(G_k e^{+2 pi i k n / 1024}) as a real inverse transform
        const int j = band_of[k];
        float dP = j >= 0 ? gb[(long)j * Tm + t] : 0.0f;
        if (k >= kLowF && k < kHighF) dP += dE;
        cf2 G = cf2{2.0f * xp[2 * k] * dP, 2.0f * xp[2 * k + 1] * dP};
        if (k == 0 || k == kN2) G = cf2{2.0f * G.x, 0.0f};
        Y[k] = G;
    }
    __syncthreads();
    for (int k = tid; k < kN2; k += 256) za[k] = irfft_pre(Y[k], Y[kN2 - k], k, tw);
    __syncthreads();
    fft_pass<4>(za, zb, kN2, kN2, 1, 1, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(zb, za, kN2, kN2, 1, 4, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(za, zb, kN2, kN2, 1, 16, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<4>(zb, za, kN2, kN2, 1, 64, tw, tid, 256, 2);
    __syncthreads();
    fft_pass<2>(za, zb, kN2, kN2, 1, 256, tw, tid, 256, 2);
    __syncthreads();
    float *out = dfr + ((long)b * Tm + t) * kWin;
    for (int n = 128 + tid; n < 384; n += 256) {  // x[2n] = Re conj(zb[n]), x[2n + 1] = Im conj(zb[n]); window positions [256, 768)
        const cf2 v = zb[n];
        out[2 * n - 256] = win[2 * n - 256] * v.x;
        out[2 * n - 255] = win[2 * n - 255] * -v.y;
    }
}

__device__ inline float frames_at(const float *df, long p, int T) {  // sum of dfr over the frames whose window covers padded position p
    float acc = 0.0f;
    const long t1 = (p + 256) >> 8;
    for (long t = t1; t >= t1 - 1 && t >= 0; t--) {
        const long j = p - t * kHop + 256;
        if (t < T && j >= 0 && j < kWin) acc += df[t * kWin + j];
    }
    return acc;
}

// grid (ceil(L / 256), B)
__global__ __launch_bounds__(256) void k_pesq_gather_bwd(const float *dfr, const int64_t *lens, long L, int Tm, float *dpred) {
    const int b = blockIdx.y;
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= L) return;
    const RowGeo g = row_geo(lens, b, L);
    float acc = 0.0f;
    if (g.ok && n < g.len) {
        const float *df = dfr + (long)b * Tm * kWin;
        acc = frames_at(df, n, g.T);
        if (n >= 1 && n <= 256) acc += frames_at(df, -n, g.T);
        const long p = 2 * (g.len - 1) - n;
        if (p >= g.len && p <= (long)(g.T - 1) * kHop + 255) acc += frames_at(df, p, g.T);
    }
    dpred[(long)b * L + n] = acc;
}

thread_local char g_pesq_err[256] = "";
int pesq_fail(const char *msg) { snprintf(g_pesq_err, sizeof g_pesq_err, "%s", msg); return SE_ERR_ARG; }

}  // namespace

extern "C" {

const char *se_loss_pesq_last_error(void) { return g_pesq_err; }

int64_t se_loss_pesq_ws_floats(int batch, int64_t length) { return batch > 0 && length > 0 ? (int64_t)pesq_shape(batch, (long)length).total : 0; }

int se_loss_pesq_fwd(const float *clean, const float *pred, const int64_t *lens, int batch, int64_t length, const float *win, const int *edges,
                     const float *band_tab, float *ws, float *value, void *stream) {
    if (!clean || !pred || !lens || !win || !edges || !band_tab || !ws || !value || batch <= 0 || batch > 65535) return pesq_fail("se_loss_pesq_fwd: bad argument");
    if (length < kMinLen) return pesq_fail("se_loss_pesq_fwd: fewer than 20 spectrogram frames (4864 samples)");
    const PesqShape s = pesq_shape(batch, (long)length);
    if (s.Tm > kMaxT) return pesq_fail("se_loss_pesq_fwd: more than 896 spectrogram frames (14.3 s) per row");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_pesq_spec, dim3(s.Tm, batch, 2), dim3(256), 0, st, clean, pred, lens, (long)length, s.Tm, win, edges, ws + s.Rt, ws + s.Rp, ws + s.lvT,
                       ws + s.lvP, ws + s.Xp);
    hipLaunchKernelGGL(k_pesq_row_fwd, dim3(batch), dim3(256), row_lds_bytes(s.Tm, s.NBm), st, ws + s.Rt, ws + s.Rp, ws + s.lvT, ws + s.lvP, lens, (long)length, s.Tm,
                       s.NBm, band_tab, reinterpret_cast<real *>(ws + s.fr), reinterpret_cast<real *>(ws + s.bd), reinterpret_cast<real *>(ws + s.sc), value);
    return hipGetLastError() == hipSuccess ? SE_OK : pesq_fail("se_loss_pesq_fwd: launch failed");
}

// ws = the workspace se_loss_pesq_fwd filled for the same inputs; gvalue [batch] = d loss / d value; dpred [batch][length]
int se_loss_pesq_bwd(const float *gvalue, const int64_t *lens, int batch, int64_t length, const float *win, const int *band_of, const float *band_tab, float *ws,
                     float *dpred, void *stream) {
    if (!gvalue || !lens || !win || !band_of || !band_tab || !ws || !dpred || batch <= 0 || batch > 65535) return pesq_fail("se_loss_pesq_bwd: bad argument");
    if (length < kMinLen) return pesq_fail("se_loss_pesq_bwd: fewer than 20 spectrogram frames (4864 samples)");
    const PesqShape s = pesq_shape(batch, (long)length);
    if (s.Tm > kMaxT) return pesq_fail("se_loss_pesq_bwd: more than 896 spectrogram frames (14.3 s) per row");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_pesq_row_bwd, dim3(batch), dim3(256), row_lds_bytes(s.Tm, s.NBm), st, ws + s.Rt, ws + s.Rp, lens, (long)length, s.Tm, s.NBm, band_tab,
                       reinterpret_cast<const real *>(ws + s.fr), reinterpret_cast<const real *>(ws + s.bd), reinterpret_cast<real *>(ws + s.sc), gvalue, ws + s.gBp,
                       ws + s.gBt);
    hipLaunchKernelGGL(k_pesq_spec_bwd, dim3(s.Tm, batch), dim3(256), 0, st, ws + s.Xp, ws + s.gBp, reinterpret_cast<const real *>(ws + s.sc), lens, (long)length, s.Tm,
                       win, band_of, ws + s.dfr);
    hipLaunchKernelGGL(k_pesq_gather_bwd, dim3((unsigned)((length + 255) / 256), batch), dim3(256), 0, st, ws + s.dfr, lens, (long)length, s.Tm, dpred);
    return hipGetLastError() == hipSuccess ? SE_OK : pesq_fail("se_loss_pesq_bwd: launch failed");
}

}  // extern "C"
