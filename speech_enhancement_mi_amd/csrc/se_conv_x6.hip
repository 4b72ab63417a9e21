// se_conv_x6.hip - k_conv_x6 template instances for ONE operand-plane count (compiled three times: -DSE_X6_PL=1, 2, 3 ->
// se_conv_x6_pl{1,2,3}.o) so that the 36 instances build in parallel.  One channel octet per chunk (CO = 1): the engine plans
// k_conv_x6 only for the multi-tap convolutions (15 taps encoder, 9 / 6 transposed even / odd parity).
#include <hip/hip_runtime.h>

#define SE_NO_NORM_KERNELS 1
#include "conv_dispatch.h"
#include "conv_x6.hip.h"

#ifndef SE_X6_PL
#error "compile with -DSE_X6_PL=1|2|3"
#endif
#define SE_CAT2(a, b) a##b
#define SE_CAT(a, b) SE_CAT2(a, b)

namespace se {

int SE_CAT(conv_x6_launch_pl, SE_X6_PL)(int ntap, int NT, dim3 grid, size_t lds, hipStream_t st, const ConvX6Args &xa) {
#define SE_X6_CASE(NTAP_, NT_) \
    case NTAP_ * 16 + NT_: hipLaunchKernelGGL((k_conv_x6<NTAP_, NT_, 1, SE_X6_PL>), grid, dim3(256), lds, st, xa); return 0;
#define SE_X6_TAPS(NTAP_) SE_X6_CASE(NTAP_, 1) SE_X6_CASE(NTAP_, 2) SE_X6_CASE(NTAP_, 3) SE_X6_CASE(NTAP_, 4)
    switch (ntap * 16 + NT) {
        SE_X6_TAPS(15) SE_X6_TAPS(9) SE_X6_TAPS(6)
        default: return 1;
    }
#undef SE_X6_TAPS
#undef SE_X6_CASE
}

void SE_CAT(conv_x6_set_attributes_pl, SE_X6_PL)() {
    const int kMax = 160 * 1024;
#define SE_X6_ATTR1(NTAP_, NT_) \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_conv_x6<NTAP_, NT_, 1, SE_X6_PL>), hipFuncAttributeMaxDynamicSharedMemorySize, kMax);
#define SE_X6_ATTR(NTAP_) SE_X6_ATTR1(NTAP_, 1) SE_X6_ATTR1(NTAP_, 2) SE_X6_ATTR1(NTAP_, 3) SE_X6_ATTR1(NTAP_, 4)
    SE_X6_ATTR(15) SE_X6_ATTR(9) SE_X6_ATTR(6)
#undef SE_X6_ATTR
#undef SE_X6_ATTR1
}

}  // namespace se
