// conv_dispatch.h - host-side entry points of the fp32-layout convolution kernels, which are compiled in their own translation
// unit (se_conv.hip) so that the engine and the kernels build in parallel.  Their launchers: the engine's vector-ALU pre-conv
// blocks (plan_conv / launch_conv in se_engine.hip) and the training path (k_conv_igemm, train_ops.inc.h); inference runs its
// encoder, its decoder and the feature-tap re-runs on k_conv_p (convp_dispatch.h).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_args.h"

namespace se {

// k_conv_igemm<NTAP, NT> (NT >= 1) or k_conv_small<NTAP, CoPad/4> (NT == 0): returns 0 on launch, 1 when no instance exists
int conv_igemm_launch(int ntap, int NT, int CoPad, dim3 grid, size_t lds, hipStream_t st, const ConvArgs &a);
void conv_set_attributes();   // opt in to large dynamic LDS for every instance

}  // namespace se
