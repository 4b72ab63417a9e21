// gemm.hip.h - dense fp32 GEMM on v_mfma_f32_32x32x2_f32 for the recurrent bottleneck (reference
// SequenceModel, CRN.py:256-282): the GRU input projections for all T frames at once
// ([B*T, in] x W_ih^T, aten::gru's first addmm) and the fc_output_layer ([B*T, H] x W_fc^T + ReLU).
//
// C[m][n] = act( sum_k A[m*lda + k] * W[n*ldw + k] + bias[n] ),  both operands K-contiguous
// (PyTorch [out, in] weights are used as they are).  128x128 block tile, 4 waves as 2x2, each wave
// 2x2 MFMA tiles of 32x32 (A and B fragments reused twice), K walked in 32-deep LDS chunks with a
// +1 row pad (conflict-free ds_read_b32 for the lane->row fragment pattern).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_igemm.hip.h"
#include "split_bf16.h"
#include "split_f16pair.h"
#include "gemm_kblock.h"

namespace se {

constexpr int kGemmBM = 128, kGemmBN = 128, kGemmKC = 32, kGemmLd = kGemmKC + 1;

struct GemmArgs {
    const float *A;
    const float *W;
    const float *bias;
    float *C;
    int M, N, K;
    long lda, ldw, ldc;
    int relu;  // activation: 0 none, 1 ReLU, 2 ELU (CRN_ELU.py:365)
};

// Stage 128 rows x 32 k of a K-contiguous operand into LDS (row stride kGemmLd).  Loads are unconditional
// 16-B loads from clamped addresses (K % 4 == 0 is enforced by the host), out-of-range values are zeroed by
// select, so the four loads of a thread are in flight together.
__device__ __forceinline__ void gemm_stage(float *dst, const float *src, long ld, int rows_valid, int row0, int k0, int K, int tid) {
    float4 q[4];
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int slot = tid + it * 256;
        const int r = slot >> 3, kq = (slot & 7) * 4;
        const int row = min(row0 + r, rows_valid - 1), k = min(k0 + kq, K - 4);
        q[it] = *reinterpret_cast<const float4 *>(src + (long)row * ld + k);
    }
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int slot = tid + it * 256;
        const int r = slot >> 3, kq = (slot & 7) * 4;
        const bool ok = (row0 + r < rows_valid) && (k0 + kq < K);
        float *d = dst + r * kGemmLd + kq;
        d[0] = ok ? q[it].x : 0.0f;
        d[1] = ok ? q[it].y : 0.0f;
        d[2] = ok ? q[it].z : 0.0f;
        d[3] = ok ? q[it].w : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_gemm_tn(GemmArgs a) {
    __shared__ float As[kGemmBM * kGemmLd];
    __shared__ float Ws[kGemmBN * kGemmLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * kGemmBM, n0 = blockIdx.x * kGemmBN;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    for (int k0 = 0; k0 < a.K; k0 += kGemmKC) {
        __syncthreads();
        gemm_stage(As, a.A, a.lda, a.M, m0, k0, a.K, tid);
        gemm_stage(Ws, a.W, a.ldw, a.N, n0, k0, a.K, tid);
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kGemmKC; kk += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; i++) av[i] = As[(wm + i * 32 + l31) * kGemmLd + kk + half];
#pragma unroll
            for (int j = 0; j < 2; j++) bv[j] = Ws[(wn + j * 32 + l31) * kGemmLd + kk + half];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // D layout: column (n) on lanes, rows (m) in registers
    float bsj[2];  // fetched ahead of all stores (a load between stores cannot be hoisted: C may alias bias)
#pragma unroll
    for (int j = 0; j < 2; j++) bsj[j] = a.bias ? a.bias[min(n0 + wn + j * 32 + l31, a.N - 1)] : 0.0f;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = n0 + wn + j * 32 + l31;
            if (n >= a.N) continue;
            const float bs = bsj[j];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < a.M) {
                    float v = acc[i][j][r] + bs;
                    v = conv_act(v, a.relu);
                    a.C[(long)m * a.ldc + n] = v;
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------
// fp32-accurate GEMM on the bf16 matrix cores ("bf16x6").  Each fp32 operand is split into three bf16 planes
// x = hi + mid + lo (24 mantissa bits, each difference exact in fp32) and the product is formed from the six
// leading cross terms hi*hi + hi*mid + mid*hi + hi*lo + lo*hi + mid*mid, accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16.  Dropped terms are <= 2^-24 relative, i.e. below fp32 rounding: measured error vs an
// fp64 GEMM 2.6e-8 (a plain fp32 k-ordered chain: 2.6e-7).  Six bf16 MFMAs (6 x 32 cycles, K = 16) replace eight
// fp32 MFMAs (8 x 64 cycles): 2.7x fewer matrix-pipe cycles, which is what bounds this path (and the chip holds
// a low clock under sustained fp32 MFMA load).
// W is pre-split on the host (three [N][K] bf16 planes); A is split on the fly while it is staged into LDS.
constexpr int kXLd = kGemmKC + 8;  // bf16 elements per LDS row (80 B: conflict-free 16-B fragment reads)

struct GemmX6Args {
    const float *A;
    const __bf16 *Wp;  // [3][N][K]
    const float *bias;
    float *C;
    int M, N, K;
    long lda, ldc;
    int relu;
};


typedef _Float16 f16x8g __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4g __attribute__((ext_vector_type(4)));

// PL = operand planes: 3 = bf16x6 (fp32-accurate), 2 = bf16x3 (hi, mid planes; se_config.precision = 2), 1 = fp16 operands
// (se_config.precision = 1); Wp then holds PL planes [PL][N][K]
template <int PL>
__global__ __launch_bounds__(256) void k_gemm_x(GemmX6Args a) {
    __shared__ __align__(16) __bf16 Ap[PL][kGemmBM * kXLd];
    __shared__ __align__(16) __bf16 Wp[PL][kGemmBN * kXLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * kGemmBM, n0 = blockIdx.x * kGemmBN;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    f32x4 qa[4];
    uint4 qw[2 * PL];
    auto issue = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int slot = tid + it * 256, r = slot >> 3, kq = (slot & 7) * 4;
            const int row = min(m0 + r, a.M - 1), k = min(k0 + kq, a.K - 4);
            qa[it] = *reinterpret_cast<const f32x4 *>(a.A + (long)row * a.lda + k);
        }
#pragma unroll
        for (int it = 0; it < 2 * PL; it++) {
            const int seg = tid + it * 256, plane = seg >> 9, w = seg & 511, r = w >> 2, q = (w & 3) * 8;
            const int row = min(n0 + r, a.N - 1), k = min(k0 + q, a.K - 8);
            qw[it] = *reinterpret_cast<const uint4 *>(a.Wp + ((long)plane * a.N + row) * a.K + k);
        }
    };
    issue(0);
    for (int k0 = 0; k0 < a.K; k0 += kGemmKC) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int slot = tid + it * 256, r = slot >> 3, kq = (slot & 7) * 4;
            const bool ok = (m0 + r < a.M) && (k0 + kq < a.K);
            if (PL >= 2) {
                bf16x4 h, m, l;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    __bf16 hh, mm, ll;
                    split3(ok ? qa[it][e] : 0.0f, hh, mm, ll);
                    h[e] = hh; m[e] = mm; l[e] = ll;
                }
                *reinterpret_cast<bf16x4 *>(&Ap[0][r * kXLd + kq]) = h;
                *reinterpret_cast<bf16x4 *>(&Ap[PL > 1 ? 1 : 0][r * kXLd + kq]) = m;
                if (PL == 3) *reinterpret_cast<bf16x4 *>(&Ap[PL > 2 ? 2 : 0][r * kXLd + kq]) = l;
            } else {
                f16x4g h;
#pragma unroll
                for (int e = 0; e < 4; e++) h[e] = (_Float16)(ok ? qa[it][e] : 0.0f);
                *reinterpret_cast<f16x4g *>(&Ap[0][r * kXLd + kq]) = h;
            }
        }
#pragma unroll
        for (int it = 0; it < 2 * PL; it++) {
            const int seg = tid + it * 256, plane = seg >> 9, w = seg & 511, r = w >> 2, q = (w & 3) * 8;
            const bool ok = (n0 + r < a.N) && (k0 + q < a.K);
            *reinterpret_cast<uint4 *>(&Wp[plane][r * kXLd + q]) = ok ? qw[it] : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        if (k0 + kGemmKC < a.K) issue(k0 + kGemmKC);  // next chunk in flight during the MFMAs
#pragma unroll
        for (int ks = 0; ks < kGemmKC; ks += 16) {
            uint4 fa[2][PL], fb[2][PL];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int p = 0; p < PL; p++) {
                    fa[i][p] = *reinterpret_cast<const uint4 *>(&Ap[p][(wm + i * 32 + l31) * kXLd + ks + half * 8]);
                    fb[i][p] = *reinterpret_cast<const uint4 *>(&Wp[p][(wn + i * 32 + l31) * kXLd + ks + half * 8]);
                }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    f32x16 c = acc[i][j];
                    if (PL >= 2) {
                        const bf16x8 a0 = __builtin_bit_cast(bf16x8, fa[i][0]), a1 = __builtin_bit_cast(bf16x8, fa[i][PL > 1 ? 1 : 0]),
                                     a2 = __builtin_bit_cast(bf16x8, fa[i][PL > 2 ? 2 : 0]);
                        const bf16x8 b0 = __builtin_bit_cast(bf16x8, fb[j][0]), b1 = __builtin_bit_cast(bf16x8, fb[j][PL > 1 ? 1 : 0]),
                                     b2 = __builtin_bit_cast(bf16x8, fb[j][PL > 2 ? 2 : 0]);
                        if (PL == 3) {
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c, 0, 0, 0);  // mid*mid
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, c, 0, 0, 0);  // hi*lo
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c, 0, 0, 0);  // lo*hi
                        }
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, c, 0, 0, 0);  // hi*mid
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, c, 0, 0, 0);  // mid*hi
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c, 0, 0, 0);  // hi*hi
                    } else {
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8g, fa[i][0]), __builtin_bit_cast(f16x8g, fb[j][0]), c, 0, 0, 0);
                    }
                    acc[i][j] = c;
                }
        }
    }
    float bsj[2];  // fetched ahead of all stores (a load between stores cannot be hoisted: C may alias bias)
#pragma unroll
    for (int j = 0; j < 2; j++) bsj[j] = a.bias ? a.bias[min(n0 + wn + j * 32 + l31, a.N - 1)] : 0.0f;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int n = n0 + wn + j * 32 + l31;
            if (n >= a.N) continue;
            const float bs = bsj[j];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < a.M) {
                    float v = acc[i][j][r] + bs;
                    v = conv_act(v, a.relu);
                    a.C[(long)m * a.ldc + n] = v;
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------
// Second-generation split-bf16 GEMM  C = act(A W^T + bias): BOTH operands arrive pre-split (A planes [PL][M][K] written by
// the producing kernel - k_gln_p for the GRU input, the GRU step's epilogue for the layer outputs; W planes [PL][N][K] from
// the host), so staging is a pure copy: `buffer_load_dwordx4 ... lds` (LDS-DMA) pieces, no VALU split, no LDS store.
//
// Shape of the kernel, and why (measured on the bottleneck GEMMs, M = 5120, N = 1536, K = 2048 / 512, all at PL = 3):
//   * these GEMMs are bound by the bytes that enter the CUs (64 B/clk/CU through the texture path), not by HBM and not by
//     the MFMA pipe: 128 x 128 tiles move 1.4 GB per launch for 77 us of MFMA work.  Three 128 x 128 variants (fp32 A split
//     in the kernel, both operands by LDS-DMA, W fragments straight from L2 into registers) all ran at 29-37 % MFMA
//     utilisation, ordered exactly by their bytes (1.2 / 1.4 / 2.2 GB -> 205 / 225 / 265 us).
//   * so the tile is 256 x 128 per CU (the largest that still gives every CU a tile: 240 tiles), 8 waves of 64 x 64 = two
//     waves per SIMD, so that one wave's DMA issue cost (60-180 cycles per 1-KiB piece) and LDS latency sit under the other
//     wave's MFMAs; 32-deep K chunks in a two-stage ring (2 x 72 KB at PL = 3): chunk kc + 1 is in flight while chunk kc is
//     multiplied, one raw s_barrier per chunk.
//   * LDS image per (operand, plane): [row][4 pieces of 16 B], piece q of row r at slot q ^ ((r >> 2) & 3): the 16-lane
//     groups of a ds_read_b128 then touch every 16-byte column of every 256-byte bank row once (conflict-free); the LDS-DMA
//     destination is lane-linear, so the permutation is applied to the SOURCE address.
//     KB (the pair's two stored weight planes on K-blocked operands, gemm_kblock.h): the image per operand is [row][8 pieces],
//     both planes of a row side by side, piece p = 4 plane + q at slot p ^ ((r >> 1) & 7).  A bank row holds two image rows; the
//     eight rows of one parity in a 16-lane group ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}) have all eight residues of r >> 1
//     mod 8, so a group again touches every 16-byte column once.  The XOR moves plane 1 to +-64 bytes from plane 0 (a per-lane
//     constant).  A wave's LDS-DMA instruction then copies 8 rows x 128 B - whole lines - where the plane-major image takes
//     16 rows x 64 B, sixteen half-used lines whose other halves are fetched again a chunk later.
//   * workgroup id -> tile is XCD-aware: the eight XCDs (id mod 8) each own a gx x gy block of tiles, so an operand tile is
//     fetched into as few L2s as possible.
struct GemmPArgs {
    const uint4 *Ap;   // [PL][M][K/8] pieces of 8 bf16 (kF16Pair: two planes of fp16)
    const uint4 *Wp;   // [PL][N][K/8]
    long a_plane, w_plane;  // uint4 per plane
    const float *bias;
    float *C;
    int M, N, K;
    long ldc;
    int relu;
    unsigned a_bytes, w_bytes;  // buffer ranges
    int nrt, nct;      // row / column tiles
    int gx, gy;        // XCD grid (gx * gy = 8, nrt % gx == 0, nct % gy == 0); gx = 0: plain row-major tile order; gx = -1: banded -
                       // XCD x (= block id mod 8) owns the gy consecutive tiles [x * gy, (x + 1) * gy) of the row-major order (a band
                       // of rows: A is fetched by one L2 apart from the band seams), for tile grids no equal 8-block split divides
    float *stats;      // optional: (sum, sum of squares) of the stored values of row m over the 128 columns of column tile ct at
                       // stats[(m * nct + ct) * 2]; rows of a stream are contiguous, so this is a SlabStats slab [b][T * nct][2]
};

constexpr int kGemmPBM = 256, kGemmPBN = 128;

#if defined(__HIP_DEVICE_COMPILE__)
#define SE_DS_READ128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
#else
#define SE_DS_READ128(dst, addr, OFF) (void)(addr)
#endif

// Sums 16 values per lane over the 32 lanes of a lane half.  Reduce-scatter: at distance n = 8, 4, 2, 1 a lane keeps the half of its
// values whose index has the lane's bit n and hands the other half to its partner; one last add joins lanes l and l ^ 16
// (16 shuffles instead of 80).  Afterwards v[0] of lane l31 is the total of index l31 & 15.  The order of the additions is fixed.
__device__ __forceinline__ void gemm_p_rowsum16(float (&v)[16], int l31) {
#pragma unroll
    for (int n = 8; n >= 1; n >>= 1) {
        // (bit selects, not `hi ? v[j + n] : v[j]`: the compiler turns that into a per-lane index into v, a 16-way compare chain)
        const unsigned hi = (l31 & n) ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int j = 0; j < n; j++) {
            const unsigned lo_b = __float_as_uint(v[j]), hi_b = __float_as_uint(v[j + n]);
            const float keep = __uint_as_float((lo_b & ~hi) | (hi_b & hi)), send = __uint_as_float((hi_b & ~hi) | (lo_b & hi));
            v[j] = keep + __shfl_xor(send, n, 64);
        }
    }
    v[0] += __shfl_xor(v[0], 16, 64);
}

// FMT = kF16Pair (split_f16pair.h; PL = 3 is then the WEIGHT plane count): A arrives as the two fp16 planes (hi, lo), W as the three
// fp16 planes (2^11 hi, lo, hi); three f16 MFMAs per tile pair accumulate 2^11 (a w) and the epilogue scales by 2^-11 ahead of the
// bias, the activation and the statistics.  The ring stage shrinks from 72 to 56 KB at the same tile.
// FMT = kF16Pair, PL = 2: the two STORED weight planes (w_lo, w_hi); 2^11 w_hi is formed from the w_hi fragments in registers, once per
// K step (pair_scale_hi), and goes into the same three MFMAs in the same order - the bits of PL = 3 from a 48 KB stage.
// KB (PL = 2 pair only): both operands K-blocked, [row][K / 32][plane][32] (gemm_kblock.h); a_plane / w_plane are unused.  Same MFMAs on
// the same fragments in the same order: the bits of the plane-major instance.
template <int PL, PlaneFmt FMT = PlaneFmt::kBf16, bool KB = false>
__global__ __launch_bounds__(512) void k_gemm_p(GemmPArgs a) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    constexpr bool kPair = FMT == PlaneFmt::kF16Pair;
    static_assert(!kPair || PL == kPairPlanesW || PL == kPairPlanesW2, "the fp16 pair has three weight planes, or two stored ones");
    constexpr bool kPairW2 = kPair && PL == kPairPlanesW2;
    static_assert(!KB || kPairW2, "K-blocked operands: the pair's two stored weight planes only");
    constexpr int PA = kPair ? kPairPlanesA : PL, PW = PL;  // planes of A / W
    extern __shared__ __align__(16) uint4 gl[];  // [stage 2]{A [PA][256 rows][4 pieces], W [PW][128 rows][4 pieces]}
    constexpr int kPieces = 1024 * PA + 512 * PW;  // uint4 per chunk
    constexpr int kNA = 2 * PA, kNW = PW;          // LDS-DMA instructions per thread per chunk for A / W
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    int rt, ct;
    if (a.gx < 0) {
        const int t = (blockIdx.x & 7) * a.gy + (blockIdx.x >> 3);
        if ((blockIdx.x >> 3) >= a.gy || t >= a.nrt * a.nct) return;  // (uniform per workgroup, ahead of every barrier)
        rt = t / a.nct;
        ct = t - rt * a.nct;
    } else if (a.gx) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const int br = a.nrt / a.gx, bc = a.nct / a.gy;  // tiles per XCD block
        rt = (xcd / a.gy) * br + slot / bc;
        ct = (xcd % a.gy) * bc + slot % bc;
    } else {
        rt = blockIdx.x / a.nct;
        ct = blockIdx.x - rt * a.nct;
    }
    const int m0 = rt * kGemmPBM, n0 = ct * kGemmPBN;
    const int wm = (wave & 3) * 64, wn = (wave >> 2) * 64;
    const int K8 = a.K >> 3, nk = a.K >> 5;
    // per-thread source offsets of chunk 0 (bytes).  A: slot s = tid + 512 i = (pl * 256 + row) * 4 + qslot (i < 2 PL);
    // W: slot s = tid + 512 i = (pl * 128 + row) * 4 + qslot (i < PL)
    unsigned voa[6], vow[3];  // (fixed extents: arrays sized by a template-dependent constant, used with the LDS-DMA builtin
                              //  inside a lambda, make clang drop the kernel's host stub without a diagnostic)
#pragma unroll
    for (int i = 0; i < kNA; i++) {
        const int s = tid + 512 * i;
        if constexpr (KB) {  // slot s = row * 8 + slot of the [256 rows][8 pieces] image; a row of the source is 2 K8 pieces
            const int row = (s >> 3) & 255;
            const long r = min(m0 + row, a.M - 1);
            voa[i] = (unsigned)((r * 2 * K8 + kblock_lds_slot(row, s & 7)) * 16);
            continue;
        }
        const int qslot = s & 3, row = (s >> 2) & 255, pl = s >> 10;
        const long r = min(m0 + row, a.M - 1);
        voa[i] = (unsigned)(((long)pl * a.a_plane + r * K8 + (qslot ^ ((row >> 2) & 3))) * 16);
    }
#pragma unroll
    for (int i = 0; i < kNW; i++) {
        const int s = tid + 512 * i;
        if constexpr (KB) {
            const int row = (s >> 3) & 127;
            const long r = min(n0 + row, a.N - 1);
            vow[i] = (unsigned)((r * 2 * K8 + kblock_lds_slot(row, s & 7)) * 16);
            continue;
        }
        const int qslot = s & 3, row = (s >> 2) & 127, pl = s >> 9;
        const long r = min(n0 + row, a.N - 1);
        vow[i] = (unsigned)(((long)pl * a.w_plane + r * K8 + (qslot ^ ((row >> 2) & 3))) * 16);
    }
    auto stage = [&](int buf, int kc) {
        // (the resources are built inside the lambda: a captured __amdgpu_buffer_rsrc_t also drops the host stub)
        const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(a.Ap), 0, a.a_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(a.Wp), 0, a.w_bytes, 0x00020000);
        const unsigned add = (unsigned)kc * (KB ? 128 : 64);  // 32 bf16 per chunk (KB: of both planes)
        uint4 *base = gl + buf * kPieces + wave * 64;
#pragma unroll
        for (int i = 0; i < kNA; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsa, (__attribute__((address_space(3))) void *)(base + i * 512), 16, voa[i] + add, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < kNW; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (__attribute__((address_space(3))) void *)(base + 1024 * PA + i * 512), 16, vow[i] + add, 0, 0, 0);
    };
    // LDS byte addresses of this lane's fragments inside one stage: rows wm + l31 / wn + l31 (+ 32 i and the plane as
    // immediates), K step ks holds pieces 2 ks + half, XOR-swizzled with bits 2-3 of the row (which only l31 contributes to)
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) void *)gl;
    const int sw = (l31 >> 2) & 3;
    unsigned adA[2], adB[2];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) {
        if constexpr (KB) {  // plane 0; rows + 32 i are immediates (4096 B), plane 1 is at + dpl
            adA[ks] = lds0 + kblock_frag_byte(wm + l31, ks, half, 0);
            adB[ks] = lds0 + (unsigned)(1024 * PA * 16) + kblock_frag_byte(wn + l31, ks, half, 0);
            continue;
        }
        adA[ks] = lds0 + (unsigned)(((wm + l31) * 4 + ((2 * ks + half) ^ sw)) * 16);
        adB[ks] = lds0 + (unsigned)((1024 * PA + (wn + l31) * 4 + ((2 * ks + half) ^ sw)) * 16);
    }
    // KB: plane 1 relative to plane 0, +64 or -64 bytes by bit 3 of the row (the same for A and B, for both K steps and both i)
    const unsigned dpl = KB ? kblock_frag_byte(l31, 0, 0, 1) - kblock_frag_byte(l31, 0, 0, 0) : 0u;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int jj = 0; jj < 2; jj++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][jj][r] = 0.0f;
    // The LDS reads are inline assembly on purpose: the compiler cannot tell a ds_read of one stage from the LDS-DMA writes
    // in flight into the other and would drain the DMA queue (s_waitcnt vmcnt(0)) in front of every visible LDS read, which
    // serialises the ring.  With opaque reads the only waits are the ones written here.
    auto multiply = [&](const u32x4 (&fa)[2][3], const u32x4 (&fb)[2][3]) {
        constexpr int P1 = PL > 1 ? 1 : 0, P2 = PL > 2 ? 2 : 0;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                f32x16 c = acc[i][jj];
                if (kPair) {  // smallest terms first, as below
                    // (kPairW2: the stored planes are (w_lo, w_hi) and slot 2 holds the 2^11 w_hi made from the second)
                    const f16x8g a0 = __builtin_bit_cast(f16x8g, fa[i][0]), a1 = __builtin_bit_cast(f16x8g, fa[i][1]);
                    const f16x8g b0 = __builtin_bit_cast(f16x8g, fb[jj][kPairW2 ? 2 : 0]), b1 = __builtin_bit_cast(f16x8g, fb[jj][kPairW2 ? 0 : 1]),
                                 b2 = __builtin_bit_cast(f16x8g, fb[jj][kPairW2 ? 1 : 2]);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b2, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, c, 0, 0, 0);
                } else if (PL >= 2) {
                    const bf16x8 a0 = __builtin_bit_cast(bf16x8, fa[i][0]), a1 = __builtin_bit_cast(bf16x8, fa[i][P1]), a2 = __builtin_bit_cast(bf16x8, fa[i][P2]);
                    const bf16x8 b0 = __builtin_bit_cast(bf16x8, fb[jj][0]), b1 = __builtin_bit_cast(bf16x8, fb[jj][P1]), b2 = __builtin_bit_cast(bf16x8, fb[jj][P2]);
                    if (PL == 3) {
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c, 0, 0, 0);
                    }
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c, 0, 0, 0);
                } else {
                    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8g, fa[i][0]), __builtin_bit_cast(f16x8g, fb[jj][0]), c, 0, 0, 0);
                }
                acc[i][jj] = c;
            }
    };
#define SE_GEMMP_READ(fa, fb, ks, sb)                               \
    if constexpr (KB) {                                             \
        const unsigned xa = adA[ks] + (sb), xb = adB[ks] + (sb);    \
        const unsigned ya = xa + dpl, yb = xb + dpl;                \
        SE_DS_READ128(fa[0][0], xa, 0);                             \
        SE_DS_READ128(fa[1][0], xa, 4096);                          \
        SE_DS_READ128(fb[0][0], xb, 0);                             \
        SE_DS_READ128(fb[1][0], xb, 4096);                          \
        SE_DS_READ128(fa[0][1], ya, 0);                             \
        SE_DS_READ128(fa[1][1], ya, 4096);                          \
        SE_DS_READ128(fb[0][1], yb, 0);                             \
        SE_DS_READ128(fb[1][1], yb, 4096);                          \
    } else {                                                        \
        const unsigned xa = adA[ks] + (sb), xb = adB[ks] + (sb);    \
        SE_DS_READ128(fa[0][0], xa, 0);                             \
        SE_DS_READ128(fa[1][0], xa, 2048);                          \
        SE_DS_READ128(fb[0][0], xb, 0);                             \
        SE_DS_READ128(fb[1][0], xb, 2048);                          \
        if constexpr (PA > 1) {                                     \
            SE_DS_READ128(fa[0][1], xa, 16384);                     \
            SE_DS_READ128(fa[1][1], xa, 16384 + 2048);              \
        }                                                           \
        if constexpr (PW > 1) {                                     \
            SE_DS_READ128(fb[0][1], xb, 8192);                      \
            SE_DS_READ128(fb[1][1], xb, 8192 + 2048);               \
        }                                                           \
        if constexpr (PA > 2) {                                     \
            SE_DS_READ128(fa[0][2], xa, 32768);                     \
            SE_DS_READ128(fa[1][2], xa, 32768 + 2048);              \
        }                                                           \
        if constexpr (PW > 2) {                                     \
            SE_DS_READ128(fb[0][2], xb, 16384);                     \
            SE_DS_READ128(fb[1][2], xb, 16384 + 2048);              \
        }                                                           \
    }
// all fragments of one K step pass through the wait, so no MFMA that consumes them can be scheduled above it
#define SE_GEMMP_WAIT(CNT, fa, fb)                                                                                             \
    if constexpr (PL == 1)                                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(" #CNT ")" : "+v"(fa[0][0]), "+v"(fa[1][0]), "+v"(fb[0][0]), "+v"(fb[1][0]));          \
    else if constexpr (PL == 2) /* (two bf16 planes, or the pair's two stored weight planes: the same eight fragments) */      \
        asm volatile("s_waitcnt lgkmcnt(" #CNT ")"                                                                             \
                     : "+v"(fa[0][0]), "+v"(fa[1][0]), "+v"(fb[0][0]), "+v"(fb[1][0]), "+v"(fa[0][1]), "+v"(fa[1][1]),         \
                       "+v"(fb[0][1]), "+v"(fb[1][1]));                                                                        \
    else if constexpr (kPair)                                                                                                  \
        asm volatile("s_waitcnt lgkmcnt(" #CNT ")"                                                                             \
                     : "+v"(fa[0][0]), "+v"(fa[1][0]), "+v"(fb[0][0]), "+v"(fb[1][0]), "+v"(fa[0][1]), "+v"(fa[1][1]),         \
                       "+v"(fb[0][1]), "+v"(fb[1][1]), "+v"(fb[0][2]), "+v"(fb[1][2]));                                        \
    else                                                                                                                       \
        asm volatile("s_waitcnt lgkmcnt(" #CNT ")"                                                                             \
                     : "+v"(fa[0][0]), "+v"(fa[1][0]), "+v"(fb[0][0]), "+v"(fb[1][0]), "+v"(fa[0][1]), "+v"(fa[1][1]),         \
                       "+v"(fb[0][1]), "+v"(fb[1][1]), "+v"(fa[0][2]), "+v"(fa[1][2]), "+v"(fb[0][2]), "+v"(fb[1][2]))
    stage(0, 0);
    for (int kc = 0; kc < nk; kc++) {
        const int buf = kc & 1;
        // chunk kc has landed; after the barrier every wave has also finished reading chunk kc - 1, whose stage chunk kc + 1
        // goes into.  The request is unconditional (past the end it re-requests the last chunk into the stage nobody reads).
        // (A third stage fits the two-plane pair's 48 KB stages - chunk kc + 2 requested here, vmcnt(kNA + kNW) left in flight - and
        // was measured: 1.3 % per launch alone and a slower pipelined step, DESIGN.md 4 round 10.  Two stages stay.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        stage(buf ^ 1, min(kc + 1, nk - 1));
        const unsigned sb = (unsigned)buf * (kPieces * 16);
#if defined(__HIP_DEVICE_COMPILE__)
        u32x4 fa0[2][3], fb0[2][3], fa1[2][3], fb1[2][3];
        SE_GEMMP_READ(fa0, fb0, 0, sb)
        SE_GEMMP_READ(fa1, fb1, 1, sb)
        if constexpr (PL == 1) { SE_GEMMP_WAIT(4, fa0, fb0); } else if constexpr (PL == 2) { SE_GEMMP_WAIT(8, fa0, fb0); } else if constexpr (kPair) { SE_GEMMP_WAIT(10, fa0, fb0); } else { SE_GEMMP_WAIT(12, fa0, fb0); }
        if constexpr (kPairW2) { fb0[0][2] = pair_scale_hi(fb0[0][1]); fb0[1][2] = pair_scale_hi(fb0[1][1]); }
        multiply(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);  // keep the first K step's MFMAs above the second wait
        SE_GEMMP_WAIT(0, fa1, fb1);
        if constexpr (kPairW2) { fb1[0][2] = pair_scale_hi(fb1[0][1]); fb1[1][2] = pair_scale_hi(fb1[1][1]); }
        multiply(fa1, fb1);
#else
        (void)sb; (void)multiply; (void)dpl;
#endif
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the tail's redundant request lands before the workgroup's LDS is released
#undef SE_GEMMP_READ
#undef SE_GEMMP_WAIT
    float bsj[2];
#pragma unroll
    for (int jj = 0; jj < 2; jj++) bsj[jj] = a.bias ? a.bias[min(n0 + wn + jj * 32 + l31, a.N - 1)] : 0.0f;
    // Optional partial statistics of the norm that follows (a.stats, uniform): per row, (sum, sum of squares) of the stored values
    // over the real columns of this tile.  The ring is free after the barrier: every wave is past its last fragment read and
    // its last DMA has landed.  The values are summed where they are stored, so the epilogue evaluates every element once.
    float *red = reinterpret_cast<float *>(gl);
    if (a.stats) __syncthreads();
    float tot[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {  // group g: rows r = 8 (g & 1) + {0..7} of M tile i = g >> 1
        const int i = g >> 1;
        float v[16];  // [0, 8): sums of the 8 rows over this lane's two columns, [8, 16): sums of squares
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int r = 8 * (g & 1) + k, m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            float ss = 0.0f, qq = 0.0f;
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const int n = n0 + wn + jj * 32 + l31;
                if (n >= a.N) continue;
                const float x = conv_act((kPair ? acc[i][jj][r] * kPairInvScale : acc[i][jj][r]) + bsj[jj], a.relu);
                if (m < a.M) a.C[(long)m * a.ldc + n] = x;
                ss += x; qq += x * x;
            }
            v[k] = ss; v[8 + k] = qq;
        }
        if (a.stats) {
            gemm_p_rowsum16(v, l31);  // lane l31: k = l31 & 7 is the row of the group, bit 3 selects sum / sum of squares
            tot[g] = v[0];
            if (wave >= 4) red[((wave & 3) * 4 + g) * 64 + lane] = v[0];
        }
    }
    if (a.stats) {
        __syncthreads();  // the two N-waves of a row meet through LDS
        if (wave < 4 && l31 < 16) {
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int r = 8 * (g & 1) + (l31 & 7), m = m0 + wm + (g >> 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < a.M) a.stats[((long)m * a.nct + ct) * 2 + ((l31 >> 3) & 1)] = tot[g] + red[(wave * 4 + g) * 64 + lane];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One GRU time step for all streams (torch.nn.GRU cell, gate order r,z,n; reference CRN.py:269):
//   gh = h_prev W_hh^T + b_hh ;  r = s(gi_r + gh_r) ; z = s(gi_z + gh_z) ; n = tanh(gi_n + r * gh_n)
//   h  = (1 - z) n + z h_prev
// gi (= x_t W_ih^T + b_ih) is precomputed for all T by k_gemm_tn.  The three gate columns of one hidden
// unit are kept in the same wave so the gate math is a register epilogue of the MFMAs (no gh round trip).
// Workgroup = 32 streams x 16 hidden units; 4 waves = 2 row tiles x 2 K halves (split-K through LDS)
// so a B=256, H=512 step exposes 256 workgroups x 4 waves = one wave per SIMD of the chip.
// v_mfma_f32_16x16x4_f32: A lane (row=l&15, k=l>>4), B lane (k=l>>4, col=l&15); each lane fetches 4
// consecutive k per 16-B load, so MFMA s of a 16-deep block contracts k = 4*(l>>4)+s on both operands.
struct GruStepArgs {
    const float *gi;     // + t*3H already applied; row stride gi_ld
    long gi_ld;
    const float *hprev;  // [B][H]
    const float *whh;    // [3H][H]
    const float *bhh;    // [3H]
    float *hout;         // [B][H]
    float *seq;          // + t*H applied; row stride seq_ld
    long seq_ld;
    int B, H;
    float *gates;        // training only (nullptr in inference): r, z, n and gh_n of this step, rows of 4H with stride gates_ld,
    long gates_ld;       // saved for the backward pass (train_ops.inc.h: k_gru_bwd_step)
    __bf16 *seqp;        // optional: h_t also as split-bf16 planes [PL][rows][H] (the A operand of the next GEMM, k_gemm_p);
    long seqp_ld, seqp_plane;  // + t*H applied; row stride and plane stride in elements
    int seqp_pl;         // planes: 3, 2, or 1 (fp16)
    int seqp_pair;       // the planes are the fp16 pair (split_f16pair.h; seqp_pl = 2) instead of bf16
    int seqp_kb;         // the pair K-blocked (gemm_kblock.h): rows of 2 H elements [H / 32][plane][32] - seqp carries + 2 t H, seqp_ld is
                         // the stride of those rows, seqp_plane = 32 and unit n sits at kblock_col(n)
};

// unit n of a row of the sequence planes (plane 0)
__device__ __forceinline__ long gru_seqp_col(const GruStepArgs &a, int n) { return a.seqp_kb ? kblock_col(n) : n; }

// h_t into the sequence planes (sp = the element of plane 0)
__device__ __forceinline__ void gru_seqp_store(const GruStepArgs &a, __bf16 *sp, float hn) {
    if (a.seqp_pair) {
        uint16_t hh, ll;
        split2h(hn, hh, ll);
        sp[0] = __builtin_bit_cast(__bf16, hh); sp[a.seqp_plane] = __builtin_bit_cast(__bf16, ll);
    } else if (a.seqp_pl == 1) {
        const _Float16 hv = (_Float16)hn;
        sp[0] = __builtin_bit_cast(__bf16, hv);
    } else {
        __bf16 hh, mm, ll;
        split3(hn, hh, mm, ll);
        sp[0] = hh; sp[a.seqp_plane] = mm;
        if (a.seqp_pl == 3) sp[2 * a.seqp_plane] = ll;
    }
}

// Up to four independent steps in ONE launch (blockIdx.z selects the argument set): the pipelined path advances layer l of
// segment n - l for every layer l at once (layer 1 lags one segment behind layer 0, so both halves of a launch have the
// same shape and no gate pre-activation has to be recomputed), which halves the chain of dependent launches per segment.
struct GruStepMulti { GruStepArgs a[4]; };

template <int NW>
__device__ __forceinline__ void gru_step_body(const GruStepArgs &a) {
    __shared__ float red[NW - 1][3][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // 32 streams per workgroup: waves = 2 row tiles x 2 halves of K.  A batch of <= 16 streams (se_step at small batch, the
    // training micro-batches) has one row tile: all four waves split K instead, which halves the chain of dependent L2 round
    // trips of a step (8 k blocks per wave instead of 16 at H = 512)
    const bool narrow = a.B <= 16;  // uniform
    const int rt = narrow ? 0 : (wave & 1), kh = narrow ? wave : (wave >> 1), nsplit = narrow ? NW : 2;  // (NW = 8 only with narrow batches)
    const int l15 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, r0 = blockIdx.y * 32 + rt * 16;
    const int H = a.H;          // multiple of 16 (host-checked): every 16-deep k block is complete
    const int nkb = H >> 4;
    const int kb0 = nkb * kh / nsplit, kb1 = nkb * (kh + 1) / nsplit;
    // out-of-range rows / hidden units read a clamped (valid) address; their results are never stored
    const int arow = min(r0 + l15, a.B - 1);
    const int n = n0 + l15;
    const int nc = min(n, H - 1);
    const float *ap = a.hprev + (long)arow * H + kq * 4;
    const float *bp0 = a.whh + (long)nc * H + kq * 4;
    const float *bp1 = bp0 + (long)H * H;
    const float *bp2 = bp1 + (long)H * H;
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
    constexpr int PF = 4;  // k blocks in flight (depth 8 measured no better: the step is bound by its L2 traffic, not by latency) (each = one L2 round trip of 4 x 16 B per lane; 16 blocks per wave at H = 512)
    float4 qa[PF], q0[PF], q1[PF], q2[PF];
#pragma unroll
    for (int i = 0; i < PF; i++) {
        const int k = min(kb0 + i, nkb - 1) * 16;
        qa[i] = *reinterpret_cast<const float4 *>(ap + k);
        q0[i] = *reinterpret_cast<const float4 *>(bp0 + k);
        q1[i] = *reinterpret_cast<const float4 *>(bp1 + k);
        q2[i] = *reinterpret_cast<const float4 *>(bp2 + k);
    }
    for (int kb = kb0; kb < kb1; kb += PF) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const float4 ca = qa[i], c0 = q0[i], c1 = q1[i], c2 = q2[i];
            const bool live = kb + i < kb1;  // uniform; a dead slot contributes nothing (halves of odd length)
            const int k = min(kb + i + PF, nkb - 1) * 16;
            qa[i] = *reinterpret_cast<const float4 *>(ap + k);
            q0[i] = *reinterpret_cast<const float4 *>(bp0 + k);
            q1[i] = *reinterpret_cast<const float4 *>(bp1 + k);
            q2[i] = *reinterpret_cast<const float4 *>(bp2 + k);
            const float s = live ? 1.0f : 0.0f;
            const float ax = ca.x * s, ay = ca.y * s, az = ca.z * s, aw = ca.w * s;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, c0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, c1.x, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ax, c2.x, acc2, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ay, c0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ay, c1.y, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ay, c2.y, acc2, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(az, c0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(az, c1.z, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(az, c2.z, acc2, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, c0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, c1.w, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw, c2.w, acc2, 0, 0, 0);
        }
    }
    // partial sums of the other K shares: slot = wave - 1 for a narrow batch (waves 1..3 -> wave 0), the row tile otherwise
    if (kh > 0) {
        const int slot = narrow ? kh - 1 : rt;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            red[slot][0][r][lane] = acc0[r];
            red[slot][1][r][lane] = acc1[r];
            red[slot][2][r][lane] = acc2[r];
        }
    }
    __syncthreads();
    if (kh == 0 && n < H) {
        const float bh_r = a.bhh[n], bh_z = a.bhh[H + n], bh_n = a.bhh[2 * H + n];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = r0 + kq * 4 + r;  // D layout: col = lane&15, row = (lane>>4)*4 + reg
            if (row >= a.B) continue;
            const int s0 = narrow ? 0 : rt;
            float p0 = red[s0][0][r][lane], p1 = red[s0][1][r][lane], p2 = red[s0][2][r][lane];
            if (narrow) {
#pragma unroll
                for (int w = 1; w < NW - 1; w++) { p0 += red[w][0][r][lane]; p1 += red[w][1][r][lane]; p2 += red[w][2][r][lane]; }
            }
            const float gh_r = acc0[r] + p0 + bh_r;
            const float gh_z = acc1[r] + p1 + bh_z;
            const float gh_n = acc2[r] + p2 + bh_n;
            const float *gi = a.gi + (long)row * a.gi_ld;
            const float rg = 1.0f / (1.0f + expf(-(gi[n] + gh_r)));
            const float zg = 1.0f / (1.0f + expf(-(gi[H + n] + gh_z)));
            const float ng = tanhf(gi[2 * H + n] + rg * gh_n);
            const float hp = a.hprev[(long)row * H + n];
            const float hn = (1.0f - zg) * ng + zg * hp;
            a.hout[(long)row * H + n] = hn;
            a.seq[(long)row * a.seq_ld + n] = hn;
            if (a.gates) {
                float *gs = a.gates + (long)row * a.gates_ld;
                gs[n] = rg; gs[H + n] = zg; gs[2 * H + n] = ng; gs[3 * H + n] = gh_n;
            }
            if (a.seqp) gru_seqp_store(a, a.seqp + (long)row * a.seqp_ld + gru_seqp_col(a, n), hn);
        }
    }
}

__global__ __launch_bounds__(256) void k_gru_step(GruStepArgs a) { gru_step_body<4>(a); }
__global__ __launch_bounds__(256) void k_gru_step_multi(GruStepMulti m) { gru_step_body<4>(m.a[blockIdx.z]); }
// batches of <= 16 streams: eight waves split K (4 k blocks each at H = 512: one round of loads in flight)
__global__ __launch_bounds__(512) void k_gru_step8(GruStepArgs a) { gru_step_body<8>(a); }
__global__ __launch_bounds__(512) void k_gru_step_multi8(GruStepMulti m) { gru_step_body<8>(m.a[blockIdx.z]); }

// Second-generation step kernel: the workgroup's W_hh slice (3 gates x 16 hidden units x H, 96 KB at H = 512) is
// staged ONCE through LDS in the exact lane order the B fragments are consumed (one conflict-free ds_read_b128 per
// fragment) and shared by the two row-tile waves, and every global load of the step (A fragments straight to
// registers, W in two batches) is issued before the first wait, so the kernel pays one memory round trip instead
// of eight dependent ones.  L2->CU traffic per step drops from 67 MB to 41 MB at B = 256.
// Requires H % 32 == 0 and 192*H bytes of LDS (host falls back to k_gru_step otherwise).
template <int NKB_HALF /* 16-deep k blocks per K half = H/32 */>
__global__ __launch_bounds__(256) void k_gru_step2(GruStepArgs a) {
    extern __shared__ __align__(16) f32x4 wlds[];  // [kb][gate][lane]
    __shared__ float red[2][3][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rt = wave & 1, kh = wave >> 1;
    const int l15 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 16, r0 = blockIdx.y * 32 + rt * 16;
    const int H = a.H;
    constexpr int NKB = 2 * NKB_HALF;
    const int arow = min(r0 + l15, a.B - 1);
    const int n = n0 + l15, nc = min(n, H - 1);
    // ---- issue every load of the step ----
    const float *ap = a.hprev + (long)arow * H + kq * 4 + kh * NKB_HALF * 16;
    f32x4 qa[NKB_HALF];
#pragma unroll
    for (int i = 0; i < NKB_HALF; i++) qa[i] = *reinterpret_cast<const f32x4 *>(ap + i * 16);
    // epilogue operands (gi is HBM/MALL resident, 129 KB row stride): fetched now, used after the MFMAs
    float pgi[4][3], php[4];
    {
        const int ncl = min(n0 + l15, H - 1);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = min(r0 + kq * 4 + r, a.B - 1);
            const float *gi = a.gi + (long)row * a.gi_ld + ncl;
            pgi[r][0] = gi[0]; pgi[r][1] = gi[H]; pgi[r][2] = gi[2 * H];
            php[r] = a.hprev[(long)row * H + ncl];
        }
    }
    // W slots: s = tid + 256*j over [kb][gate][lane]; stage 0 holds the first half of each K half so both
    // halves can start after one batch: kb order = {0..h/2-1, h..h+h/2-1 | h/2..h-1, h+h/2..2h-1}
    constexpr int SLOTS = NKB * 3 * 64 / 256;  // float4 per thread (24 at H = 512)
    constexpr int HS = SLOTS / 2;
    f32x4 qw[SLOTS];
    const float *wrow = a.whh + (long)nc * H + kq * 4;
    auto kb_of = [&](int ord) {  // ord in [0, NKB): position in the staged order -> k block
        const int stage = ord / NKB_HALF, r = ord % NKB_HALF;          // NKB_HALF blocks per stage
        const int khalf = r / (NKB_HALF / 2), q = r % (NKB_HALF / 2);  // half of them from each K half
        return khalf * NKB_HALF + stage * (NKB_HALF / 2) + q;
    };
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        const int s = wave + 4 * j;            // (ord, gate) pair index: 64 lanes of a wave fill one fragment
        const int ord = s / 3, g = s - ord * 3;
        const int kb = kb_of(ord);
        qw[j] = *reinterpret_cast<const f32x4 *>(wrow + (long)g * H * H + kb * 16);
    }
    // ---- stage 0 -> LDS ----
#pragma unroll
    for (int j = 0; j < HS; j++) {
        const int s = wave + 4 * j;
        const int ord = s / 3, g = s - ord * 3;
        wlds[(kb_of(ord) * 3 + g) * 64 + lane] = qw[j];
    }
    __syncthreads();
    f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
    auto run = [&](int i0, int i1) {
#pragma unroll
        for (int i = i0; i < i1; i++) {
            const int kb = kh * NKB_HALF + i;
            const f32x4 c0 = wlds[(kb * 3 + 0) * 64 + lane], c1 = wlds[(kb * 3 + 1) * 64 + lane], c2 = wlds[(kb * 3 + 2) * 64 + lane];
            const f32x4 ca = qa[i];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[e], c0[e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[e], c1[e], acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[e], c2[e], acc2, 0, 0, 0);
            }
        }
    };
    run(0, NKB_HALF / 2);
    // ---- stage 1 -> LDS (disjoint slots: no barrier needed before the writes) ----
#pragma unroll
    for (int j = HS; j < SLOTS; j++) {
        const int s = wave + 4 * j;
        const int ord = s / 3, g = s - ord * 3;
        wlds[(kb_of(ord) * 3 + g) * 64 + lane] = qw[j];
    }
    __syncthreads();
    run(NKB_HALF / 2, NKB_HALF);
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            red[rt][0][r][lane] = acc0[r];
            red[rt][1][r][lane] = acc1[r];
            red[rt][2][r][lane] = acc2[r];
        }
    }
    __syncthreads();
    if (kh == 0 && n < H) {
        const float bh_r = a.bhh[n], bh_z = a.bhh[H + n], bh_n = a.bhh[2 * H + n];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = r0 + kq * 4 + r;  // D layout: col = lane&15, row = (lane>>4)*4 + reg
            if (row >= a.B) continue;
            const float gh_r = acc0[r] + red[rt][0][r][lane] + bh_r;
            const float gh_z = acc1[r] + red[rt][1][r][lane] + bh_z;
            const float gh_n = acc2[r] + red[rt][2][r][lane] + bh_n;
            const float rg = 1.0f / (1.0f + expf(-(pgi[r][0] + gh_r)));
            const float zg = 1.0f / (1.0f + expf(-(pgi[r][1] + gh_z)));
            const float ng = tanhf(pgi[r][2] + rg * gh_n);
            const float hp = php[r];
            const float hn = (1.0f - zg) * ng + zg * hp;
            a.hout[(long)row * H + n] = hn;
            a.seq[(long)row * a.seq_ld + n] = hn;
            if (a.seqp) gru_seqp_store(a, a.seqp + (long)row * a.seqp_ld + gru_seqp_col(a, n), hn);
        }
    }
}

// Third-generation step kernel, for the plane route at PL = 3: the recurrent contraction on the bf16 matrix cores as the six
// split-bf16 products of k_gemm_p (same term order, smallest first) instead of v_mfma_f32_16x16x4_f32.
//   A  the planes of h_{t-1}: for t >= 1 they are already in memory - row t - 1 of the sequence planes the previous step's epilogue
//      wrote (`hp`); at t = 0 (`hp` null) the fp32 `hprev` is split on the fly.  split3 is exact, so both give the same operand bits
//      and no plane state is carried between calls.
//   B  W_hh packed by the host (gru_pack.h): [unit group][k step][gate][plane] fragments of 64 lanes x 16 bytes.
// Workgroup = 32 * MT streams x 32 hidden units, v_mfma_f32_32x32x16_bf16, one accumulator tile per gate and row tile.  ONE wave
// covers all the workgroup's streams, so every W fragment is loaded once per workgroup; the four waves split K and each keeps PF k
// steps of operands in flight.  The partial sums meet through LDS one gate at a time (reduce-scatter: wave w ends up with rows
// 8 w .. 8 w + 7 of each row tile, 12 KB * MT, summed in one order for every row), so all four waves share the epilogue.
// Requires H % 32 == 0 (host-checked).
// Measured at B = 256, H = 512: MT = 1, PF = 2 (152 VGPRs + 48 AGPRs, 12 KB LDS, no scratch) takes 11.4 us
// per single-layer launch alone against 12.0 (k_gru_step2) and 14.5 (k_gru_step), 21 us instead of 34 per two-layer launch under
// overlap, and the pipelined step 52.5 -> 48.9 ms.  On one box PF = 4 (296 registers) took 12.3 us alone and 49.8 ms per step where
// PF = 2 took 11.5 and 48.2, and MT = 2 - 64 streams per workgroup, 310 registers, 24 KB - 17.4 us and 49.1 ms: the step is bound
// by its chain of dependent L2 round trips and by what it takes from the co-resident convolutions, not by MFMA issue (1.9 us) or
// bytes (50 MB per launch).
struct GruSplitArgs {
    GruStepArgs s;        // as k_gru_step (gates unused; seqp is required: 3 bf16 planes, or the fp16 pair with PAIR)
    const uint4 *whp;     // packed W_hh planes
    const __bf16 *hp;     // planes of h_{t-1}: s.seqp - H for t >= 1, nullptr at t = 0
};
struct GruSplitMulti { GruSplitArgs a[4]; };

// PAIR: the fp16 pair format (split_f16pair.h) - two A planes from `hp` (at t = 0 split2h on the fly, which gives the bits the previous
// epilogue would have stored), W_hh packed as (2^11 hi, lo, hi) fp16 fragments in the same image, three f16 MFMAs per gate, the
// 2^-11 applied to the reduced sums ahead of the bias, h_t stored as two planes.  Same split-K reduction order.
// WPL = 2 (PAIR only): W_hh packed with the two stored planes (w_lo, w_hi) per gate - six fragments per k step instead of nine; 2^11 w_hi
// is made from the w_hi fragment when the slot is multiplied (pair_scale_hi), so the MFMAs see the operands of WPL = 3.
// Measured at B = 256, H = 512: 9.73 us per single-layer launch alone against 10.38 with nine fragments; with the
// smaller ring PF = 2 is 119 VGPRs, PF = 3 151 and PF = 4 183 - 9.87 and 9.95 us alone, no gain in the pipelined step - so PF = 2 stays.
template <int MT, int PF, bool PAIR = false, int WPL = 3>
__device__ __forceinline__ void gru_split_body(const GruSplitArgs &ga) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    static_assert(WPL == 3 || (PAIR && WPL == kPairPlanesW2), "three weight planes, or the fp16 pair's two stored ones");
    constexpr int NA = PAIR ? kPairPlanesA : 3;  // A planes
    constexpr int NWF = 3 * WPL;                 // W fragments per k step
    __shared__ float red[4][3][MT * 4][64];  // [source wave][destination wave, the source left out][register][lane]
    const GruStepArgs &a = ga.s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int H = a.H, KS = H >> 4;
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * (32 * MT);
    if (r0 >= a.B) return;  // (uniform, ahead of every barrier: a layer of a multi launch with fewer rows than the grid covers)
    const int n = n0 + l31;  // < H: the grid is exactly H / 32 wide
    const int ks0 = KS * wave / 4, ks1 = KS * (wave + 1) / 4;
    // ---- epilogue operands: requested now, used after the MFMAs.  Wave w, register i, row tile mt: row 32 mt + 8 w + 4 half + i
    float pgi[MT][4][3], php[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = min(r0 + mt * 32 + 8 * wave + 4 * half + i, a.B - 1);  // (clamped rows are never stored)
            const float *gi = a.gi + (long)row * a.gi_ld + n;
            pgi[mt][i][0] = gi[0]; pgi[mt][i][1] = gi[H]; pgi[mt][i][2] = gi[2 * H];
            php[mt][i] = a.hprev[(long)row * H + n];
        }
    const float bh_r = a.bhh[n], bh_z = a.bhh[H + n], bh_n = a.bhh[2 * H + n];
    // ---- operand streams.  One request pattern for both sources of A (a branch here would make the compiler index the operand
    // ring at run time and spill it): plane p of a k step at abase[p] + ks * astride.  At t = 0 the raw fp32 values travel in
    // slots 0 and 1 (slot 2 repeats slot 1) and are split when they are used.
    const bool planes = ga.hp != nullptr;  // uniform
    const char *abase[MT][NA];
    const long astride = planes ? 32 : 64;  // bytes per k step: 16 bf16 / 16 floats
    // K-blocked planes (seqp_kb): a 32-deep block of a row is one 128-byte line [plane][32], so k step ks starts (ks >> 1) * 64 bytes
    // further on and a lane's two planes are two 16-byte runs of the same line (seqp_plane = 32 elements)
    const long akb = planes && a.seqp_kb ? 64 : 0;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int arow = min(r0 + mt * 32 + l31, a.B - 1);
        const char *pb = reinterpret_cast<const char *>((planes ? ga.hp : a.seqp) + (long)arow * a.seqp_ld + half * 8);
        const char *fb = reinterpret_cast<const char *>(a.hprev + (long)arow * H + half * 8);
#pragma unroll
        for (int p = 0; p < NA; p++) abase[mt][p] = planes ? pb + p * a.seqp_plane * 2 : fb + (p ? 16 : 0);
    }
    const uint4 *wp = ga.whp + (long)blockIdx.x * KS * NWF * 64 + lane;
    u32x4 qa[PF][MT][NA], qw[PF][NWF];
    auto request = [&](int i, int ks) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int p = 0; p < NA; p++) qa[i][mt][p] = *reinterpret_cast<const u32x4 *>(abase[mt][p] + ks * astride + (ks >> 1) * akb);
#pragma unroll
        for (int f = 0; f < NWF; f++) qw[i][f] = *reinterpret_cast<const u32x4 *>(wp + ((long)ks * NWF + f) * 64);
    };
    f32x16 acc[MT][3];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int g = 0; g < 3; g++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][g][r] = 0.0f;
#pragma unroll
    for (int i = 0; i < PF; i++) request(i, min(ks0 + i, KS - 1));
    for (int ks = ks0; ks < ks1; ks += PF) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            // a slot past the wave's share (shares that are no multiple of PF) holds a valid k step and is multiplied by zero:
            // no branch around the MFMAs, which would send the accumulators through a copy on every trip
            const unsigned keep = ks + i < ks1 ? 0xFFFFFFFFu : 0u;  // uniform
            u32x4 ca[MT][NA];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                if (!planes && PAIR) {
                    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
                    u16x8 hh, ll;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float x = __uint_as_float(e < 4 ? qa[i][mt][0][e & 3] : qa[i][mt][1][e & 3]);
                        uint16_t h1, l1;
                        split2h(x, h1, l1);
                        hh[e] = h1; ll[e] = l1;
                    }
                    ca[mt][0] = __builtin_bit_cast(u32x4, hh);
                    ca[mt][1] = __builtin_bit_cast(u32x4, ll);
                } else if (!planes) {
                    bf16x8 hh, mm, ll;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const float x = __uint_as_float(e < 4 ? qa[i][mt][0][e & 3] : qa[i][mt][1][e & 3]);
                        __bf16 h1, m1, l1;
                        split3(x, h1, m1, l1);
                        hh[e] = h1; mm[e] = m1; ll[e] = l1;
                    }
                    ca[mt][0] = __builtin_bit_cast(u32x4, hh);
                    ca[mt][1] = __builtin_bit_cast(u32x4, mm);
                    ca[mt][NA - 1] = __builtin_bit_cast(u32x4, ll);  // (NA = 3 on this branch)
                } else {
#pragma unroll
                    for (int p = 0; p < NA; p++) ca[mt][p] = qa[i][mt][p];
                }
#pragma unroll
                for (int p = 0; p < NA; p++) ca[mt][p] &= keep;
            }
            u32x4 w0[3];  // WPL = 2: 2^11 w_hi of the three gates, once per k step (dead otherwise)
            if constexpr (WPL == 2) {
#pragma unroll
                for (int g = 0; g < 3; g++) w0[g] = pair_scale_hi(qw[i][g * 2 + 1]);
            }
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                if constexpr (PAIR) {
                    const f16x8g a0 = __builtin_bit_cast(f16x8g, ca[mt][0]), a1 = __builtin_bit_cast(f16x8g, ca[mt][1]);
#pragma unroll
                    for (int g = 0; g < 3; g++) {
                        const f16x8g b0 = __builtin_bit_cast(f16x8g, WPL == 2 ? w0[g] : qw[i][g * WPL]), b1 = __builtin_bit_cast(f16x8g, qw[i][g * WPL + (WPL == 2 ? 0 : 1)]),
                                     b2 = __builtin_bit_cast(f16x8g, qw[i][g * WPL + WPL - 1]);
                        f32x16 c = acc[mt][g];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b2, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, c, 0, 0, 0);
                        acc[mt][g] = c;
                    }
                } else {
                    const bf16x8 a0 = __builtin_bit_cast(bf16x8, ca[mt][0]), a1 = __builtin_bit_cast(bf16x8, ca[mt][1]), a2 = __builtin_bit_cast(bf16x8, ca[mt][NA - 1]);
#pragma unroll
                    for (int g = 0; g < 3; g++) {
                        const bf16x8 b0 = __builtin_bit_cast(bf16x8, qw[i][g * WPL]), b1 = __builtin_bit_cast(bf16x8, qw[i][g * WPL + 1]), b2 = __builtin_bit_cast(bf16x8, qw[i][g * WPL + WPL - 1]);
                        f32x16 c = acc[mt][g];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c, 0, 0, 0);
                        acc[mt][g] = c;
                    }
                }
            }
            // the slot's next k step, requested behind the MFMAs that read the slot (nothing past the wave's share)
            if (ks + i + PF < ks1) request(i, ks + i + PF);
        }
    }
    // ---- split-K reduction, one gate per round through the same 12 KB * MT: a wave hands registers 4 d .. 4 d + 3 of the gate's
    // tiles to wave d and adds the four shares of its own registers in wave order 0, 1, 2, 3 - the same order for every row, so a
    // stream's bits do not depend on its place in the batch
    float gh[MT][3][4];
#pragma unroll
    for (int g = 0; g < 3; g++) {
        float own[MT][4];
        if (g) __syncthreads();  // the previous round has been read
#pragma unroll
        for (int d = 0; d < 4; d++) {
            if (d == wave) {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int i = 0; i < 4; i++) own[mt][i] = acc[mt][g][4 * d + i];
            } else {
                const int slot = d - (d > wave ? 1 : 0);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int i = 0; i < 4; i++) red[wave][slot][mt * 4 + i][lane] = acc[mt][g][4 * d + i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; s++) {
            float v[MT][4];
            if (s == wave) {
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int i = 0; i < 4; i++) v[mt][i] = own[mt][i];
            } else {
                const int slot = wave - (wave > s ? 1 : 0);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int i = 0; i < 4; i++) v[mt][i] = red[s][slot][mt * 4 + i][lane];
            }
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int i = 0; i < 4; i++) gh[mt][g][i] = s ? gh[mt][g][i] + v[mt][i] : v[mt][i];
        }
    }
    // ---- gate math and stores: D layout col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), reg >> 2 = wave here
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = r0 + mt * 32 + 8 * wave + 4 * half + i;
            if (row >= a.B) continue;
            const float gh_r = (PAIR ? gh[mt][0][i] * kPairInvScale : gh[mt][0][i]) + bh_r;
            const float gh_z = (PAIR ? gh[mt][1][i] * kPairInvScale : gh[mt][1][i]) + bh_z;
            const float gh_n = (PAIR ? gh[mt][2][i] * kPairInvScale : gh[mt][2][i]) + bh_n;
            const float rg = 1.0f / (1.0f + expf(-(pgi[mt][i][0] + gh_r)));
            const float zg = 1.0f / (1.0f + expf(-(pgi[mt][i][1] + gh_z)));
            const float ng = tanhf(pgi[mt][i][2] + rg * gh_n);
            const float hn = (1.0f - zg) * ng + zg * php[mt][i];
            a.hout[(long)row * H + n] = hn;
            a.seq[(long)row * a.seq_ld + n] = hn;
            __bf16 *sp = a.seqp + (long)row * a.seqp_ld + gru_seqp_col(a, n);
            if constexpr (PAIR) {
                uint16_t hh, ll;
                split2h(hn, hh, ll);
                sp[0] = __builtin_bit_cast(__bf16, hh); sp[a.seqp_plane] = __builtin_bit_cast(__bf16, ll);
            } else {
                __bf16 hh, mm, ll;
                split3(hn, hh, mm, ll);
                sp[0] = hh; sp[a.seqp_plane] = mm; sp[2 * a.seqp_plane] = ll;
            }
        }
}

template <int MT, int PF, bool PAIR = false, int WPL = 3>
__global__ __launch_bounds__(256) void k_gru_step_split(GruSplitArgs a) { gru_split_body<MT, PF, PAIR, WPL>(a); }
template <int MT, int PF, bool PAIR = false, int WPL = 3>
__global__ __launch_bounds__(256) void k_gru_step_split_multi(GruSplitMulti m) { gru_split_body<MT, PF, PAIR, WPL>(m.a[blockIdx.z]); }

}  // namespace se
