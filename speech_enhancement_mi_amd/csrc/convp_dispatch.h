// convp_dispatch.h - host entry points of the plane-layout convolution path (conv_p.hip.h), compiled in se_convp*.o.
#pragma once
#include <hip/hip_runtime.h>
#include "conv_p_args.h"
#include "split_f16pair.h"

namespace se {

// k_conv_p<NTAP, NT, CO, PL[, NTAP2][, FMT]> (ntap2 = 0: one tap list): 0 = launched, 1 = no such instance.  fmt = the format of the
// INPUT buffer (and of a P-layout output): kF16Pair instances exist for 15, 9 (+ 6), 6 and 1 taps at PL = 3 and at PL = 2, PL being
// the STORED weight planes of the pair there (split_f16pair.h)
int conv_p_launch(int ntap, int ntap2, int NT, int CO, int PL, dim3 grid, size_t lds, hipStream_t st, const ConvPArgs &a,
                  PlaneFmt fmt = PlaneFmt::kBf16);
bool conv_p_has_instance(int ntap, int NT, int CO, int ntap2 = 0);
void conv_p_set_attributes();
void launch_k_featurize_p(int PL, dim3 grid, hipStream_t st, const FeatPArgs &a);
// fmt = kF16Pair: the output planes are the fp16 pair (PL is then not used)
void launch_k_gln_p(int PL, dim3 grid, hipStream_t st, const GlnPArgs &a, PlaneFmt fmt = PlaneFmt::kBf16);
void launch_k_f32_to_p(int PL, dim3 grid, hipStream_t st, const F32ToPArgs &a);
void launch_k_gln2_p(int PL, dim3 grid, hipStream_t st, const Gln2PArgs &a, PlaneFmt fmt = PlaneFmt::kBf16);
void launch_k_gln2_stream_p(int PL, dim3 grid, hipStream_t st, const Gln2PArgs &a, PlaneFmt fmt = PlaneFmt::kBf16);
void launch_k_final_mask_p(dim3 grid, hipStream_t st, const MaskPArgs &a);
// k_skip_p<PL, KP[, FMT]> (skip_p.hip.h): one workgroup per stream; 0 = launched, 1 = no such instance.  fmt = the format of res and out
// (kF16Pair: PL = the stored weight planes, 2 or 3)
int launch_k_skip_p(int PL, int KP, int batch, size_t lds, hipStream_t st, const struct SkipPArgs &a, PlaneFmt fmt = PlaneFmt::kBf16, int depth = 0);
void skip_p_set_attributes();

}  // namespace se
