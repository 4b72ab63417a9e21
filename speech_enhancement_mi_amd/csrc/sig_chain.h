// sig_chain.h - the STFT signal chain of one geometry: the Hamming window, the twiddle table, the overlap-add envelope and the FFT plan,
// on one device, and the two launchers of k_stft / k_istft (stft.hip.h).  The CRN engine, the FullSubNet engine (se_engine.hip) and the
// training signal handle se_sig (se_train.hip) each own one; defined in se_aux.hip next to the kernels' launchers, so every unit of the
// library links against one table builder and one place that fills StftArgs / IstftArgs.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "stft.hip.h"

namespace se {

struct MaskPArgs;  // conv_p_args.h

struct SigChain {
    int device = 0, N = 0, win = 0, hop = 0, K = 0, T = 0, F = 0;  // n_fft, window, hop, segment samples, frames 1 + K/hop, bins N/2 + 1
    float *window = nullptr, *env = nullptr, *tw = nullptr;        // device: hamming(win) centred in N [N]; sum_t w^2 [K]; exp(-2 pi i m / N) [N] (cf2)
    FftPlan plan{};
};

// Validates the geometry, builds and uploads the tables on `device` and opts the FFT kernels in to the LDS they need (a K whose LDS need
// exceeds the chip's is accepted: such a chain is never launched, aux_set_fft_lds).  SE_OK, or an SE_ERR_* code with its text in err and
// nothing left allocated.
int sig_chain_create(SigChain &s, int n_fft, int win, int hop, int K, int device, std::string &err);
void sig_chain_destroy(SigChain &s);

// Per-stream lengths and first-segment offsets of a chains call (device int64 [rows / M]); both null: every row has Lsrc samples from `off`.
struct SigRows {
    const long *len = nullptr, *off0 = nullptr;
};

// rows = streams x M waveform rows, row r at src + (r / M) * strideB + (r % M) * strideM; sample k of segment y reads
// src[row + rows.off0[r / M] + off + y * seg_off + k] inside [0, min(Lsrc, rows.len[r / M])), zero outside; element (row, t, f) of
// segment y -> spec[y * seg_spec + row * sR + t * sT + f * sF].  Returns the launch's error.
hipError_t sig_stft(const SigChain &s, const float *src, long strideB, long strideM, int M, long off, long Lsrc, SigRows rows, int nrows, cf2 *spec,
                    long sR, long sT, long sF, hipStream_t st, int nseg = 1, long seg_off = 0, long seg_spec = 0);
// the inverse: segment y of row r -> wav[y * seg_wav + r * wav_ld + (0 .. K)]
hipError_t sig_istft(const SigChain &s, const cf2 *spec, long sR, long sT, long sF, int nrows, float *wav, long wav_ld, hipStream_t st, int nseg = 1,
                     long seg_spec = 0, long seg_wav = 0);

// The CRN engine's fused ends (io_fused.hip.h), one segment per launch.
// sig_stft_feat: the STFT of all M <= 4 microphones of `nstreams` streams (addressing and zero fill as sig_stft, rows = streams); microphone
// 0's spectrum -> spec0[b * sB + t * sT + f * sF], the feature octets -> feat[b * feat_stream + ...] in the P layout of PL planes.
hipError_t sig_stft_feat(const SigChain &s, const float *src, long strideB, long strideM, int M, long off, long Lsrc, SigRows rows, int nstreams,
                         cf2 *spec0, long sB, long sT, long sF, uint4 *feat, long feat_stream, int PL, int atan2_phase, hipStream_t st);
// sig_mask_istft: m as for k_final_mask_p (its `out` is not used); stream b -> wav[b * wav_ld + (0 .. K)]
hipError_t sig_mask_istft(const SigChain &s, const MaskPArgs &m, int nstreams, float *wav, long wav_ld, hipStream_t st);
// whether the two kernels' workgroups fit the LDS of a CU at this geometry (the engine keeps the four-kernel route otherwise)
bool sig_io_fused_fits(const SigChain &s, int M);

}  // namespace se
