// fsn_train.hip.h - kernels of FullSubNet training (fsn_train_fwd / fsn_train_bwd, include/se_engine.h; reference
// train_fullsubnet.py:137-145 = torch autograd over realtime_process(train=False), fullsubnet.py:769-824, 903-961).
//
//   k_fsn_save_rows   training forward: a per-window tensor (element (r, t, k) at src[r*sR + t*sT + k]) into the [T][S][W] layout
//   k_lstm_bwd_step   one BPTT step of one LSTM layer for ALL windows' sequences: dh_rec = dG_{t+1} W_hh as an fp32-exact MFMA GEMM
//                     (M = S rows, N = H units, K = 4H), the LSTM cell backward in the epilogue
//   k_fsn_gather_dm   d crm [N][B][2][F][T] -> d mask [T][S][2] (the sub-band output layer's gradient, rows of the backward layout:
//                     dense, or packed through a row table)
//   k_fsn_dfb         d fb_out: column SI - 1 of the sub-band input gradient (dG_0 . W_ih_l0[:, SI - 1]) / that window's CumLayerNorm
//                     denominator (the running mean is detached, fullsubnet.py:200), through the full-band ReLU
// Every sum has a fixed order (no float atomics): the gradients are bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>

namespace se {

__global__ void k_fsn_save_rows(const float *src, long sR, long sT, int W, int R, int T, float *dst, long dT) {
    const long total = (long)T * R * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i / ((long)R * W));
        const long q = i - (long)t * R * W;
        const int r = (int)(q / W), k = (int)(q - (long)r * W);
        dst[(long)t * dT + (long)r * W + k] = src[(long)r * sR + (long)t * sT + k];
    }
}

// ---- one BPTT step -----------------------------------------------------------------------------------------------------------
// Saved forward values of step t (torch.nn.LSTM cell, gate order i, f, g, o): c_t = f c_{t-1} + i g, h_t = o tanh(c_t).
//   dh   = dout_t + dG_{t+1} W_hh                    (dout_t: the loss / next layer; dm . W_fc for the sub-band output layer)
//   dc   = dh o (1 - tanh^2 c_t) + dc_{t+1} f_{t+1}  (`dcf` carries dc_{t+1} f_{t+1} in and dc_t f_t out, in place)
//   dG_t = [dc g i(1-i), dc c_{t-1} f(1-f), dc i (1-g^2), dh tanh(c_t) o(1-o)]
// GEMM: 128 x 128 tile (rows x units) per workgroup, four waves as 2 x 2 of 64 x 64 (2 x 2 accumulators of v_mfma_f32_32x32x2_f32),
// K = 4H in 32-deep chunks through LDS, the next chunk's global loads in flight during the current chunk's MFMAs.  Within an
// 8-deep k block lane half h contracts k = 4h .. 4h + 3 of both operands (one 16-byte LDS read per operand per block), the order
// k_gemm_skinny uses.  W_hh is passed transposed ([H][4H], K-contiguous) so both operands stage the same way.
struct LstmBwdArgs {
    const float *dgn;    // dG_{t+1} [S][4H], nullptr at the last step (no recurrent term, dcf not read)
    const float *whh_t;  // [H][4H]
    const float *dout;   // [S][H] or nullptr
    const float *dm;     // [S][2] or nullptr: d of the output layer Linear(H -> 2) of this step, with its weight wfc [2][H]
    const float *wfc;
    const float *gates;  // [S][4H] post-activation i, f, g, o of step t
    const float *cprev, *ccur;  // [S][H] c_{t-1}, c_t
    float *dcf;          // [S][H]
    float *dg;           // [S][4H] out
    int S, H;
};
constexpr int kLbwBM = 128, kLbwBN = 128, kLbwKC = 32, kLbwLd = kLbwKC + 4;

__global__ __launch_bounds__(256) void k_lstm_bwd_step(LstmBwdArgs a) {
    __shared__ __align__(16) float As[kLbwBM * kLbwLd];
    __shared__ __align__(16) float Bs[kLbwBN * kLbwLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const int m0 = blockIdx.y * kLbwBM, n0 = blockIdx.x * kLbwBN;
    const int H = a.H, K = 4 * H;  // H % 8 == 0 (host-checked): K is a multiple of the 32-deep chunk
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    if (a.dgn) {
        const int nck = K / kLbwKC;
        // This thread's four 16-byte slots of each operand chunk: row / unit r_it = (tid >> 3) + 32 it, k offset kq.  Plain unrolled
        // loops over named registers, no by-reference lambda: the prefetch registers stay in VGPRs (a lambda-captured array was
        // demoted to scratch, which serialised every chunk's global loads in front of its MFMAs).
        const int kq = (tid & 7) * 4;
        const float *pa[4], *pb[4];
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int r = (tid >> 3) + 32 * it;
            pa[it] = a.dgn + (long)min(m0 + r, a.S - 1) * K + kq;   // clamped rows / units are computed and never stored
            pb[it] = a.whh_t + (long)min(n0 + r, H - 1) * K + kq;
        }
        float4 qa0 = *reinterpret_cast<const float4 *>(pa[0]), qa1 = *reinterpret_cast<const float4 *>(pa[1]);
        float4 qa2 = *reinterpret_cast<const float4 *>(pa[2]), qa3 = *reinterpret_cast<const float4 *>(pa[3]);
        float4 qb0 = *reinterpret_cast<const float4 *>(pb[0]), qb1 = *reinterpret_cast<const float4 *>(pb[1]);
        float4 qb2 = *reinterpret_cast<const float4 *>(pb[2]), qb3 = *reinterpret_cast<const float4 *>(pb[3]);
        const int ra = tid >> 3;
        for (int ck = 0; ck < nck; ck++) {
            __syncthreads();  // every wave is done reading the previous chunk
            *reinterpret_cast<float4 *>(&As[(ra + 0) * kLbwLd + kq]) = qa0;
            *reinterpret_cast<float4 *>(&As[(ra + 32) * kLbwLd + kq]) = qa1;
            *reinterpret_cast<float4 *>(&As[(ra + 64) * kLbwLd + kq]) = qa2;
            *reinterpret_cast<float4 *>(&As[(ra + 96) * kLbwLd + kq]) = qa3;
            *reinterpret_cast<float4 *>(&Bs[(ra + 0) * kLbwLd + kq]) = qb0;
            *reinterpret_cast<float4 *>(&Bs[(ra + 32) * kLbwLd + kq]) = qb1;
            *reinterpret_cast<float4 *>(&Bs[(ra + 64) * kLbwLd + kq]) = qb2;
            *reinterpret_cast<float4 *>(&Bs[(ra + 96) * kLbwLd + kq]) = qb3;
            __syncthreads();
            // the next chunk's loads go out before this chunk's MFMAs (the last iteration re-reads its own chunk: no branch, unused)
            const long kn = (long)min(ck + 1, nck - 1) * kLbwKC;
            qa0 = *reinterpret_cast<const float4 *>(pa[0] + kn); qa1 = *reinterpret_cast<const float4 *>(pa[1] + kn);
            qa2 = *reinterpret_cast<const float4 *>(pa[2] + kn); qa3 = *reinterpret_cast<const float4 *>(pa[3] + kn);
            qb0 = *reinterpret_cast<const float4 *>(pb[0] + kn); qb1 = *reinterpret_cast<const float4 *>(pb[1] + kn);
            qb2 = *reinterpret_cast<const float4 *>(pb[2] + kn); qb3 = *reinterpret_cast<const float4 *>(pb[3] + kn);
            __builtin_amdgcn_sched_barrier(0);  // hipcc otherwise sinks these loads to the next iteration's head, in front of the LDS stores
#pragma unroll
            for (int kb = 0; kb < kLbwKC / 8; kb++) {
                float4 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    fa[i] = *reinterpret_cast<const float4 *>(&As[(wm + i * 32 + l31) * kLbwLd + kb * 8 + 4 * kh]);
                    fb[i] = *reinterpret_cast<const float4 *>(&Bs[(wn + i * 32 + l31) * kLbwLd + kb * 8 + 4 * kh]);
                }
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        f32x16 c = acc[i][j];
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, c, 0, 0, 0);
                        acc[i][j] = c;
                    }
            }
        }
    }
    // epilogue: D layout column (unit) on the lane, rows (r & 3) + 8 (r >> 2) + 4 kh
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int u = n0 + wn + j * 32 + l31;
        if (u >= H) continue;
        const float w0 = a.dm ? a.wfc[u] : 0.0f, w1 = a.dm ? a.wfc[H + u] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (m >= a.S) continue;
                const long idx = (long)m * H + u;
                float dh = acc[i][j][r];
                if (a.dout) dh += a.dout[idx];
                if (a.dm) dh += a.dm[2 * (long)m] * w0 + a.dm[2 * (long)m + 1] * w1;
                const float *g = a.gates + (long)m * 4 * H;
                const float ig = g[u], fg = g[H + u], gg = g[2 * H + u], og = g[3 * H + u];
                const float tc = tanhf(a.ccur[idx]);
                float dc = dh * og * (1.0f - tc * tc);
                if (a.dgn) dc += a.dcf[idx];
                float *d = a.dg + (long)m * 4 * H;
                d[u] = dc * gg * ig * (1.0f - ig);
                d[H + u] = dc * a.cprev[idx] * fg * (1.0f - fg);
                d[2 * H + u] = dc * ig * (1.0f - gg * gg);
                d[3 * H + u] = dh * tc * og * (1.0f - og);
                a.dcf[idx] = dc * fg;
            }
    }
}

// dm[t][s][c] = dcrm[n][b][c][f][t], s = p*F + f over the S0 rows p of the backward layout: p = n*B + b (rowmap null, the dense
// layout) or rowmap[p] = n*B + b (the packed layout of a chains call, which leaves the dead windows out)
__global__ void k_fsn_gather_dm(const float *dcrm, float *dm, const int *rowmap, long S0, int F, int T) {
    const long S = S0 * F, total = (long)T * S * 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i & 1);
        const long q = i >> 1;
        const int t = (int)(q / S);
        const long s = q - (long)t * S;
        const long p = s / F;
        const int f = (int)(s - p * F);
        const long nb = rowmap ? rowmap[p] : p;
        dm[i] = dcrm[((nb * 2 + c) * F + f) * T + t];
    }
}

// dpre[t][p][f] (row stride Fp, columns >= F untouched) = relu'(fb_out) * (sum_g dG0[t][p*F + f][g] * wcol[g]) / denom[p], p = the
// S0 rows of the backward layout (dense n*B + b, or packed): denom, fbo and dpre are all indexed by p
// one wave per (t, p, f); lanes across g, a fixed shuffle tree
__global__ __launch_bounds__(256) void k_fsn_dfb(const float *dg0, const float *wcol, const float *denom, const float *fbo, float *dpre,
                                                 long S0, int F, int T, int H4, int Fp) {
    const int lane = threadIdx.x & 63;
    const long wid = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((long)gridDim.x * blockDim.x) >> 6;
    const long Ssb = S0 * F, total = (long)T * Ssb;
    for (long row = wid; row < total; row += nw) {
        const float *g = dg0 + row * H4;
        float s = 0.0f;
        for (int k = lane; k < H4; k += 64) s += g[k] * wcol[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) {
            const int t = (int)(row / Ssb);
            const long q = row - (long)t * Ssb, p = q / F;
            const int f = (int)(q - p * F);
            const long r = (long)t * S0 + p;  // row of the full-band layout [T][S0]
            dpre[r * Fp + f] = fbo[r * F + f] > 0.0f ? s / denom[p] : 0.0f;
        }
    }
}

}  // namespace se
