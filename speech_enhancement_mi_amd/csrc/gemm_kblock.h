// gemm_kblock.h - the K-blocked layout of the fp16 pair's GEMM operands (k_gemm_p<2, kF16Pair, true>, gemm.hip.h).
//
// Plane-major operands ([plane][row][K] fp16) give k_gemm_p 64 bytes per (row, plane) and 32-deep chunk: one LDS-DMA wave instruction
// copies 16 rows x 64 B, sixteen half-used 128-byte lines, and the other half of each line is fetched a chunk later by another
// instruction.  K-blocked, both planes of a 32-deep K block of one row are contiguous,
//     [row][K / 32][plane][32] fp16          one 128-byte line per (row, block),
// and a wave instruction copies 8 rows x 128 B: whole lines.  The layout is a property of the buffer (engine_host.h:
// buffer_kblocked): the GEMM A buffers (gruinP, seqP) and the weights k_gemm_p reads (W_ih0, W_ih1.., fc_output_layer), only where the
// pair is on with its two stored weight planes.  Every other route keeps plane-major.
// Plain C++ on the host (the engine's weight upload and tests/gemm_kblock_check.cpp compile the same code); the index helpers are
// shared with the kernels.
#pragma once
#include <vector>
#include "split_f16pair.h"

namespace se {

constexpr int kKbBlock = 32;  // fp16 per plane and block: the chunk depth of k_gemm_p (kGemmKC)

// element offset of column k inside a K-blocked row, plane 0; plane p adds p * kKbBlock.  A row holds 2 K elements.
SE_PAIR_HD inline long kblock_col(long k) { return (k >> 5) * (2 * kKbBlock) + (k & 31); }
// element index of (row, k, plane) in a K-blocked [rows][K] pair operand
SE_PAIR_HD inline long kblock_index(long row, long K, long k, int plane) { return row * 2 * K + kblock_col(k) + (long)plane * kKbBlock; }

// ---- the LDS image of one operand in a ring stage of k_gemm_p: [row][8 pieces of 16 B], 128 bytes per row.
// Logical piece p of a row = 8 fp16 of its line: pieces 0-3 are plane 0 (k = 8 p ..), pieces 4-7 plane 1.  Piece p of row r sits
// in slot p ^ ((r >> 1) & 7).  Why this is conflict-free: a ds_read_b128 is served in four groups of 16 lanes, lanes
// {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of each wave half, and its banks span 256 bytes = two rows of the image.  A lane reads
// row = its index in the half (+ a multiple of 16), all lanes of a group the same logical piece.  The 16-byte column a lane touches is
// 8 (r & 1) + slot.  The eight rows of one parity in a group have r >> 1 = {0, 1, 6, 7, 10, 11, 12, 13} or {2, 3, 4, 5, 8, 9, 14, 15}:
// all residues mod 8, so the XOR sends them to the eight different slots, and the two parities take the two halves of the bank row.
// The XOR reaches bit 2 of the piece, so the planes of a row trade places in half of the rows: plane 1 of a fragment is at +64 or
// -64 bytes from plane 0, by bit 3 of the row (a per-lane constant), not at an immediate offset.
// The LDS-DMA destination is lane-linear, so the permutation is applied to the SOURCE address: the lane that fills slot s of row r
// fetches logical piece s ^ ((r >> 1) & 7) - the XOR is its own inverse.  The eight lanes of a row still cover one whole line.
SE_PAIR_HD inline int kblock_lds_slot(int row, int piece) { return piece ^ ((row >> 1) & 7); }
// byte offset, inside one operand's image, of the fragment a lane reads: row, K step ks (16 deep), lane half, plane
SE_PAIR_HD inline unsigned kblock_frag_byte(int row, int ks, int half, int plane) {
    return (unsigned)((row * 8 + kblock_lds_slot(row, 4 * plane + 2 * ks + half)) * 16);
}

// a [rows][K] weight matrix as the K-blocked image of its two stored planes (w_lo, w_hi): defined through pair_weight_matrix2, so there
// is one definition of the split
inline void pair_weight_matrix2_kblock(const float *w, size_t rows, size_t K, uint16_t *out) {
    const size_t n = rows * K;
    std::vector<uint16_t> planes(2 * n);
    pair_weight_matrix2(w, n, planes.data());
    for (size_t r = 0; r < rows; r++)
        for (size_t k = 0; k < K; k++)
            for (int p = 0; p < kPairPlanesW2; p++) out[kblock_index((long)r, (long)K, (long)k, p)] = planes[(size_t)p * n + r * K + k];
}

}  // namespace se
