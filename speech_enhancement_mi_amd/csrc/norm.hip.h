// norm.hip.h - per-stream global layer norm and the pointwise stages fused around it.
//
// Reference: GlobalLayerNorm(time=False).forward (CRN.py:135-149): per sample, mean and BIASED variance
// over every non-batch element (two passes, like the reference), y = (x - mu) / (sqrt(var + 1e-8) + 1e-8) * w + b.
// One workgroup (1024 threads = 16 wavefronts) owns one stream's tensor (<= ~180 KB, L2 resident after
// the first pass); reductions are wavefront shuffles + one LDS hop, combined in double.
// Fused variants (fp32 layout; the plane path's norms are in conv_p.hip.h):
//   k_featurize  - |X|, arctan phase differences (CRN.py:463-467)
//   k_gln_ew     - norm + affine (+ residual add, + re-layout) from the producing conv's partial statistics
//   k_gln_r2t    - the same from the plane path's R layout into the bottleneck GEMM's [T][C*F] rows
#pragma once
#include <hip/hip_runtime.h>
#include "fft_lds.h"

namespace se {

constexpr float kEps = 1e-8f;  // CRN.py:11

// gLN denominator: sqrt(var + eps) + eps (CRN.py:149, CRN_ELU.py:51) or sqrt(var) + eps (distillation_crn.py:51)
__device__ __forceinline__ float gln_inv(float var, int eps_outside_only) {
    return 1.0f / ((eps_outside_only ? sqrtf(var) : sqrtf(var + kEps)) + kEps);
}

__device__ inline double block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();  // protect red from a previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < nw; i++) s += red[i];
    return s;
}

// mean and 1/(sqrt(var+eps)+eps) of n contiguous floats (two-pass, biased variance)
__device__ inline void stream_stats(const float *x, long n, double *red, float &mean, float &inv, int eps_mode = 0) {
    float part = 0.0f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) part += x[i];
    const double s = block_sum((double)part, red);
    mean = (float)(s / (double)n);
    float p2 = 0.0f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = x[i] - mean;
        p2 += d * d;
    }
    const double q = block_sum((double)p2, red);
    const float var = (float)(q / (double)n);
    inv = gln_inv(var, eps_mode);
}

// ---- featurise: spec (b, m, t, f) -> feat [B][2M-1][T][F] --------------------------------------
struct FeatArgs {
    const cf2 *spec;
    long sB, sM, sT, sF;  // strides in cf2 units
    float *feat;
    int M, T, F;
    int atan2_phase;  // 0: arctan(im/(re+eps)+eps) (CRN.py:464, distillation_crn.py:340); 1: atan2(im, re) (CRN_ELU.py:370)
};

#if !defined(SE_AUX_KERNELS) && !defined(SE_NO_NORM_KERNELS)
__global__ void k_featurize(FeatArgs a) {
    const int b = blockIdx.y;
    const int TF = a.T * a.F;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= TF) return;
    const int t = i / a.F, f = i - t * a.F;
    const cf2 *s = a.spec + (long)b * a.sB + (long)t * a.sT + (long)f * a.sF;
    float *o = a.feat + (long)b * (2 * a.M - 1) * TF + i;
    float ang0 = 0.0f;
    for (int m = 0; m < a.M; m++) {
        const cf2 v = s[(long)m * a.sM];
        o[(long)m * TF] = sqrtf(v.x * v.x + v.y * v.y + 1e-10f);
        const float ang = a.atan2_phase ? atan2f(v.y, v.x) : atanf(v.y / (v.x + kEps) + kEps);
        if (m == 0) ang0 = ang;
        else o[(long)(a.M + m - 1) * TF] = ang0 - ang;
    }
}

#endif  // norm kernels

// ---- cIRM decompression (utility.py:439-442) --------------------------------------------------------------
__device__ inline float decompress_cirm(float m) {
    m = m >= 9.9f ? 9.9f : (m <= -9.9f ? -9.9f : m);
    return -10.0f * logf((10.0f - m) / (10.0f + m));
}

// ---- elementwise variants: statistics come from the producing convolution's per-workgroup partials ----------
// (one pass over the tensor instead of three, full-chip grid instead of one workgroup per stream)
struct SlabStats { const float *slab; int nslot; long n; int eps_mode; };  // slab [B][nslot][2] = (sum, sum of squares)

__device__ __forceinline__ void slab_mean_inv(const SlabStats &st, int b, float *sm /*[2] shared*/, float &mean, float &inv) {
    if (threadIdx.x < 64) {
        double s = 0, q = 0;
        const float *p = st.slab + (long)b * st.nslot * 2;
        for (int i = threadIdx.x; i < st.nslot; i += 64) { s += (double)p[2 * i]; q += (double)p[2 * i + 1]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); q += __shfl_down(q, off, 64); }
        if (threadIdx.x == 0) {
            const double m = s / (double)st.n;
            double var = q / (double)st.n - m * m;
            if (var < 0) var = 0;
            sm[0] = (float)m;
            sm[1] = gln_inv((float)var, st.eps_mode);
        }
    }
    __syncthreads();
    mean = sm[0];
    inv = sm[1];
}

struct GlnEwArgs {
    const float *x;
    float *y;
    const float *w, *b;
    SlabStats st;
    int mode;  // 0: [C][T][F] -> same | 1: [C][T][F] -> [T][C*F]
    int C, T, F;
    const float *res;  // mode 0 only: y = gLN(x) + res (the `m(x) + x` of the preconv blocks, CRN_ELU.py:375-376)
};

// VW = 4: float4 path (n % 4 == 0, so every stream's base stays 16-B aligned); VW = 1: scalar path for odd sizes
// (the 5-channel preconv tensors of CRN_ELU: 5*21*201 elements).
#if !defined(SE_AUX_KERNELS) && !defined(SE_NO_NORM_KERNELS)
template <int VW>
__global__ __launch_bounds__(256) void k_gln_ew(GlnEwArgs a) {
    __shared__ float sm[2];
    const int b = blockIdx.y;
    float mean, inv;
    slab_mean_inv(a.st, b, sm, mean, inv);
    const long n = a.st.n;
    const float *x = a.x + (long)b * n;
    float *y = a.y + (long)b * n;
    const float *res = a.res ? a.res + (long)b * n : nullptr;
    const int TF = a.T * a.F, F = a.F, C = a.C;
    const float invTF = 1.0f / (float)TF;
    for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VW; i < n; i += (long)gridDim.x * blockDim.x * VW) {
        float vv[VW], o[VW];
        int cc[VW];
        if (VW == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(x + i);
            vv[0] = v.x; vv[VW > 1 ? 1 : 0] = v.y; vv[VW > 2 ? 2 : 0] = v.z; vv[VW > 3 ? 3 : 0] = v.w;
        } else {
            vv[0] = x[i];
        }
#pragma unroll
        for (int k = 0; k < VW; k++) {
            int c = (int)(((float)(i + k) + 0.5f) * invTF);  // (i+k) / TF, exact for n < 2^22
            c = min(c, C - 1);
            cc[k] = c;
            o[k] = (vv[k] - mean) * inv * a.w[c] + a.b[c];
        }
        if (a.mode == 0) {
            if (VW == 4) {
                if (res) {
                    const float4 r4 = *reinterpret_cast<const float4 *>(res + i);
                    o[0] += r4.x; o[VW > 1 ? 1 : 0] += r4.y; o[VW > 2 ? 2 : 0] += r4.z; o[VW > 3 ? 3 : 0] += r4.w;
                }
                *reinterpret_cast<float4 *>(y + i) = make_float4(o[0], o[VW > 1 ? 1 : 0], o[VW > 2 ? 2 : 0], o[VW > 3 ? 3 : 0]);
            } else {
                y[i] = o[0] + (res ? res[i] : 0.0f);
            }
        } else {
#pragma unroll
            for (int k = 0; k < VW; k++) {
                const int r = (int)(i + k) - cc[k] * TF, t = r / F, f = r - t * F;
                y[((long)t * C + cc[k]) * F + f] = o[k];
            }
        }
    }
}

#endif  // norm kernels

// R layout (conv_p.hip.h: [b][octet][t*F + f][8] fp32) -> normalised [T][C*F] fp32 rows, the A operand of the bottleneck's input
// GEMM (CRN.py:476-478: reshape [B, C, F, T] -> [B, C*F, T] -> permute); one thread per (octet, position)
#if !defined(SE_AUX_KERNELS) && !defined(SE_NO_NORM_KERNELS)
__global__ __launch_bounds__(256) void k_gln_r2t(GlnEwArgs a, long x_stream) {
    __shared__ float sm[2];
    const int b = blockIdx.y;
    float mean, inv;
    slab_mean_inv(a.st, b, sm, mean, inv);
    const int TF = a.T * a.F, C8 = (a.C + 7) / 8;
    const float *x = a.x + (long)b * x_stream;
    float *y = a.y + (long)b * a.st.n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < C8 * TF; i += gridDim.x * 256) {
        const int o = i / TF, pos = i - o * TF, t = pos / a.F, f = pos - t * a.F;
        const float4 *src = reinterpret_cast<const float4 *>(x + ((long)o * TF + pos) * 8);
        const float4 u0 = src[0], u1 = src[1];
        const float v[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int ch = o * 8 + c;
            if (ch < a.C) y[((long)t * a.C + ch) * a.F + f] = (v[c] - mean) * inv * a.w[ch] + a.b[ch];
        }
    }
}
#endif  // norm kernels

}  // namespace se
