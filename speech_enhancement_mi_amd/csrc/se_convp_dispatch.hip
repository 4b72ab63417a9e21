// se_convp_dispatch.hip - routes conv_p_launch() to the per-(planes, taps) translation units of se_convp.hip.
#include <hip/hip_runtime.h>

#define SE_NO_NORM_KERNELS 1
#include "convp_dispatch.h"

namespace se {

#define SE_DECL(PL_, NT_)                                                                                                  \
    int conv_p_launch_pl##PL_##_t##NT_(int ntap2, int NT, int CO, dim3 grid, size_t lds, hipStream_t st, const ConvPArgs &a); \
    void conv_p_set_attributes_pl##PL_##_t##NT_();
#define SE_DECL3(NT_) SE_DECL(1, NT_) SE_DECL(2, NT_) SE_DECL(3, NT_)
SE_DECL3(25) SE_DECL3(15) SE_DECL3(9) SE_DECL3(6) SE_DECL3(1)

#define SE_DECLP(NT_)                                                                                                  \
    int conv_p_launch_pair_t##NT_(int ntap2, int NT, int CO, dim3 grid, size_t lds, hipStream_t st, const ConvPArgs &a); \
    void conv_p_set_attributes_pair_t##NT_();                                                                          \
    int conv_p_launch_pair2_t##NT_(int ntap2, int NT, int CO, dim3 grid, size_t lds, hipStream_t st, const ConvPArgs &a); \
    void conv_p_set_attributes_pair2_t##NT_();
SE_DECLP(15) SE_DECLP(9) SE_DECLP(6) SE_DECLP(1)

int conv_p_launch(int ntap, int ntap2, int NT, int CO, int PL, dim3 grid, size_t lds, hipStream_t st, const ConvPArgs &a, PlaneFmt fmt) {
    if (fmt == PlaneFmt::kF16Pair) {  // (PL = the STORED weight planes, 2 or 3; the instances of se_convp.hip's pair section)
#define SE_ROUTEP(NT_) \
    if (ntap == NT_) return PL == kPairPlanesW2 ? conv_p_launch_pair2_t##NT_(ntap2, NT, CO, grid, lds, st, a) : conv_p_launch_pair_t##NT_(ntap2, NT, CO, grid, lds, st, a);
        SE_ROUTEP(15) SE_ROUTEP(9) SE_ROUTEP(6) SE_ROUTEP(1)
        return 1;
    }
#define SE_ROUTE(PL_, NT_) \
    if (PL == PL_ && ntap == NT_) return conv_p_launch_pl##PL_##_t##NT_(ntap2, NT, CO, grid, lds, st, a);
#define SE_ROUTE3(NT_) SE_ROUTE(1, NT_) SE_ROUTE(2, NT_) SE_ROUTE(3, NT_)
    SE_ROUTE3(25) SE_ROUTE3(15) SE_ROUTE3(9) SE_ROUTE3(6) SE_ROUTE3(1)
    return 1;
}

bool conv_p_has_instance(int ntap, int NT, int CO, int ntap2) {
    if (ntap2) return ntap == 9 && ntap2 == 6 && CO == 1 && NT >= 1 && NT <= 3;  // (PL >= 2 only: see se_convp.hip)
    const bool nt_ok = NT == 1 || NT == 2 || NT == 3 || NT == 4 || NT == 6 || NT == 8 || NT == 10 || NT == 12;
    if (!nt_ok) return false;
    if (ntap == 1) return CO == 1 || CO == 2 || CO == 4;
    if (ntap == 25) return CO == 1 && NT <= 4;
    return (ntap == 15 || ntap == 9 || ntap == 6) && CO == 1;
}

void conv_p_set_attributes() {
#define SE_ATTR(PL_, NT_) conv_p_set_attributes_pl##PL_##_t##NT_();
#define SE_ATTR3(NT_) SE_ATTR(1, NT_) SE_ATTR(2, NT_) SE_ATTR(3, NT_)
    SE_ATTR3(25) SE_ATTR3(15) SE_ATTR3(9) SE_ATTR3(6) SE_ATTR3(1)
    conv_p_set_attributes_pair_t15(); conv_p_set_attributes_pair_t9(); conv_p_set_attributes_pair_t6(); conv_p_set_attributes_pair_t1();
    conv_p_set_attributes_pair2_t15(); conv_p_set_attributes_pair2_t9(); conv_p_set_attributes_pair2_t6(); conv_p_set_attributes_pair2_t1();
}

}  // namespace se
