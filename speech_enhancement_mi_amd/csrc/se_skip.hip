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

// One instance per (format, planes, K steps, activation): the activation is a template parameter of the gate, so that the ReLU
// instances carry no ELU code.  launch: 0 = launched, 1 = no such instance; attributes only: the dynamic LDS limit of the instance.
template <int PL, int KP, int ACT, PlaneFmt FMT>
static void skip_instance(bool batched, bool attributes_only, int batch, size_t lds, hipStream_t st, const SkipPArgs &a, int depth) {
    constexpr int WPL = FMT == PlaneFmt::kF16Pair ? kPairPlanesW : PL;  // (the two-stored-plane instances keep the wave count of the
    constexpr int NWP = SE_SK_NW(WPL, KP), NWD = SE_SKD_NW(WPL, KP);    //  three-plane ones: they hold the same three weight operands)
    if (attributes_only) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_p<PL, KP, NWP, ACT, FMT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_skip_pd<PL, KP, NWD, ACT, FMT>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    } else if (batched) {
        hipLaunchKernelGGL((k_skip_pd<PL, KP, NWD, ACT, FMT>), dim3(batch), dim3(NWD * 64), lds, st, a, depth);
    } else {
        hipLaunchKernelGGL((k_skip_p<PL, KP, NWP, ACT, FMT>), dim3(batch), dim3(NWP * 64), lds, st, a);
    }
}

template <int PL, PlaneFmt FMT>
static int skip_dispatch(int KP, int act, bool batched, bool attributes_only, int batch, size_t lds, hipStream_t st, const SkipPArgs &a, int depth) {
#define SE_SKI(KP_, ACT_) \
    if (KP == KP_ && act == ACT_) { skip_instance<PL, KP_, ACT_, FMT>(batched, attributes_only, batch, lds, st, a, depth); return 0; }
    SE_SKI(1, 1) SE_SKI(2, 1) SE_SKI(4, 1) SE_SKI(1, 2) SE_SKI(2, 2) SE_SKI(4, 2)
#undef SE_SKI
    return 1;
}

static int skip_dispatch(int PL, PlaneFmt fmt, int KP, int act, bool batched, bool attributes_only, int batch, size_t lds, hipStream_t st, const SkipPArgs &a, int depth) {
    if (fmt == PlaneFmt::kF16Pair) {
        if (PL == kPairPlanesW) return skip_dispatch<kPairPlanesW, PlaneFmt::kF16Pair>(KP, act, batched, attributes_only, batch, lds, st, a, depth);
        if (PL == kPairPlanesW2) return skip_dispatch<kPairPlanesW2, PlaneFmt::kF16Pair>(KP, act, batched, attributes_only, batch, lds, st, a, depth);
        return 1;
    }
    if (PL == 1) return skip_dispatch<1, PlaneFmt::kBf16>(KP, act, batched, attributes_only, batch, lds, st, a, depth);
    if (PL == 2) return skip_dispatch<2, PlaneFmt::kBf16>(KP, act, batched, attributes_only, batch, lds, st, a, depth);
    if (PL == 3) return skip_dispatch<3, PlaneFmt::kBf16>(KP, act, batched, attributes_only, batch, lds, st, a, depth);
    return 1;
}

// depth = 0: k_skip_p, the one-ahead loop; depth >= 1: k_skip_pd with batches of min(depth, capacity) tiles; depth < 0: the default -
// k_skip_pd at its capacity for KP = 1 and 4, k_skip_p for KP = 2: alone the batched KP = 2 instance is 2 us faster, but its 218
// registers (129 before) leave no room for a second kernel's waves on the CU, and the pipelined step loses 1 %.
// a.act (1 ReLU, 2 ELU) selects the instance; any other value has none.
int launch_k_skip_p(int PL, int KP, int batch, size_t lds, hipStream_t st, const SkipPArgs &a, PlaneFmt fmt, int depth) {
    if (depth < 0) depth = KP == 2 ? 0 : 1 << 20;
    return skip_dispatch(PL, fmt, KP, a.act, depth > 0, false, batch, lds, st, a, depth);
}

void skip_p_set_attributes() {
    const SkipPArgs none{};
    for (PlaneFmt fmt : {PlaneFmt::kBf16, PlaneFmt::kF16Pair})
        for (int PL : {1, 2, 3})
            for (int KP : {1, 2, 4})
                for (int act : {1, 2}) (void)skip_dispatch(PL, fmt, KP, act, false, true, 0, 0, nullptr, none, 0);
}

}  // namespace se
