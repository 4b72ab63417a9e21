// se_skip.hip - translation unit of the streaming skip-gate kernel (skip_p.hip.h).
#include <hip/hip_runtime.h>

#define SE_NO_NORM_KERNELS 1
#include "convp_dispatch.h"
#include "skip_p.hip.h"

namespace se {

// waves per workgroup from KP x planes: 16 (1024 threads, 128 registers) up to 4, 8 above.  The fp16 pair form counts its three WEIGHT
// planes, as the three-plane bf16 form does: with 16 waves its KP = 2 instance, two activation planes in flight, still needs 12 bytes
// of scratch per lane in 128 registers (compiler report); with 8 waves it takes what it needs and KP = 1 / 2 / 4 are all scratch-free.
#define SE_SK_NW(PL_, KP_) (KP_ * PL_ <= 4 ? 16 : 8)

// the batched form (k_skip_pd): 8 waves and 256 registers, so that a wave's whole share of res fits one batch and stays in registers
// (KEEP); 16 waves for KP = 1, which is bound by VALU issue and needs the four waves per SIMD (8 waves: 81 instead of 61 us per launch)
#define SE_SKD_NW(PL_, KP_) (KP_ == 1 ? 16 : 8)

// depth = 0: k_skip_p, the one-ahead loop; depth >= 1: k_skip_pd with batches of min(depth, capacity) tiles; depth < 0: the default -
// k_skip_pd at its capacity for KP = 1 and 4, k_skip_p for KP = 2: alone the batched KP = 2 instance is 2 us faster, but its 218
// registers (129 before) leave no room for a second kernel's waves on the CU, and the pipelined step loses 1 %
int launch_k_skip_p(int PL, int KP, int batch, size_t lds, hipStream_t st, const SkipPArgs &a, PlaneFmt fmt, int depth) {
    if (depth < 0) depth = KP == 2 ? 0 : 1 << 20;
    if (depth > 0) {
#define SE_SKDP(WPL_, KP_) \
    if (PL == WPL_ && KP == KP_) { hipLaunchKernelGGL((k_skip_pd<WPL_, KP_, SE_SKD_NW(kPairPlanesW, KP_), PlaneFmt::kF16Pair>), dim3(batch), dim3(SE_SKD_NW(kPairPlanesW, KP_) * 64), lds, st, a, depth); return 0; }
        if (fmt == PlaneFmt::kF16Pair) {
            SE_SKDP(kPairPlanesW, 1) SE_SKDP(kPairPlanesW, 2) SE_SKDP(kPairPlanesW, 4)
            SE_SKDP(kPairPlanesW2, 1) SE_SKDP(kPairPlanesW2, 2) SE_SKDP(kPairPlanesW2, 4)
            return 1;
        }
#define SE_SKD(PL_, KP_) \
    if (PL == PL_ && KP == KP_) { hipLaunchKernelGGL((k_skip_pd<PL_, KP_, SE_SKD_NW(PL_, KP_)>), dim3(batch), dim3(SE_SKD_NW(PL_, KP_) * 64), lds, st, a, depth); return 0; }
#define SE_SKD3(KP_) SE_SKD(1, KP_) SE_SKD(2, KP_) SE_SKD(3, KP_)
        SE_SKD3(1) SE_SKD3(2) SE_SKD3(4)
        return 1;
    }
    // (the two-stored-plane instances keep the wave count of the three-plane ones: they hold the same three weight operands per K step)
#define SE_SKP(WPL_, KP_) \
    if (PL == WPL_ && KP == KP_) { hipLaunchKernelGGL((k_skip_p<WPL_, KP_, SE_SK_NW(kPairPlanesW, KP_), PlaneFmt::kF16Pair>), dim3(batch), dim3(SE_SK_NW(kPairPlanesW, KP_) * 64), lds, st, a); return 0; }
    if (fmt == PlaneFmt::kF16Pair) {
        SE_SKP(kPairPlanesW, 1) SE_SKP(kPairPlanesW, 2) SE_SKP(kPairPlanesW, 4)
        SE_SKP(kPairPlanesW2, 1) SE_SKP(kPairPlanesW2, 2) SE_SKP(kPairPlanesW2, 4)
        return 1;
    }
#define SE_SK(PL_, KP_) \
    if (PL == PL_ && KP == KP_) { hipLaunchKernelGGL((k_skip_p<PL_, KP_, SE_SK_NW(PL_, KP_)>), dim3(batch), dim3(SE_SK_NW(PL_, KP_) * 64), lds, st, a); return 0; }
#define SE_SK3(KP_) SE_SK(1, KP_) SE_SK(2, KP_) SE_SK(3, KP_)
    SE_SK3(1) SE_SK3(2) SE_SK3(4)
    return 1;
}

void skip_p_set_attributes() {
#define SE_SKA(PL_, KP_) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_p<PL_, KP_, SE_SK_NW(PL_, KP_)>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
#define SE_SKA3(KP_) SE_SKA(1, KP_) SE_SKA(2, KP_) SE_SKA(3, KP_)
    SE_SKA3(1) SE_SKA3(2) SE_SKA3(4)
#define SE_SKAP(WPL_, KP_) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_p<WPL_, KP_, SE_SK_NW(kPairPlanesW, KP_), PlaneFmt::kF16Pair>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    SE_SKAP(kPairPlanesW, 1) SE_SKAP(kPairPlanesW, 2) SE_SKAP(kPairPlanesW, 4)
    SE_SKAP(kPairPlanesW2, 1) SE_SKAP(kPairPlanesW2, 2) SE_SKAP(kPairPlanesW2, 4)
#define SE_SKDA(PL_, KP_) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_pd<PL_, KP_, SE_SKD_NW(PL_, KP_)>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
#define SE_SKDA3(KP_) SE_SKDA(1, KP_) SE_SKDA(2, KP_) SE_SKDA(3, KP_)
    SE_SKDA3(1) SE_SKDA3(2) SE_SKDA3(4)
#define SE_SKDAP(WPL_, KP_) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_pd<WPL_, KP_, SE_SKD_NW(kPairPlanesW, KP_), PlaneFmt::kF16Pair>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    SE_SKDAP(kPairPlanesW, 1) SE_SKDAP(kPairPlanesW, 2) SE_SKDAP(kPairPlanesW, 4)
    SE_SKDAP(kPairPlanesW2, 1) SE_SKDAP(kPairPlanesW2, 2) SE_SKDAP(kPairPlanesW2, 4)
}

}  // namespace se
