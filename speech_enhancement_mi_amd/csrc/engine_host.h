// engine_host.h - the host plumbing the two inference engines (se_engine, fsn_engine: se_engine.hip and its .inc.h files) share: the
// error text, checked HIP calls, device buffers, the split-bf16 / fp16 operand planes of a weight matrix, the parameter table and the
// upload of a chains call's plan.  Plain inline host code, one translation unit's worth.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/se_engine.h"
#include "chain_plan.h"
#include "split_f16pair.h"
#include "gemm_kblock.h"

namespace se {

struct EngineHost {  // base of se_engine and fsn_engine
    std::string err;  // what *_last_error(e) returns
    int device = 0;
    std::map<std::string, std::vector<float>> params;  // host copies by canonical key
};

inline thread_local std::string g_create_error;  // *_last_error(NULL): why the last create on this thread failed

inline int fail(EngineHost *e, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    (e ? e->err : g_create_error) = buf;
    return code;
}

#define HIPCHECK(e, call)                                                                      \
    do {                                                                                       \
        hipError_t _st = (call);                                                               \
        if (_st != hipSuccess)                                                                 \
            return fail(e, SE_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_st), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

struct DevBuf {
    float *p = nullptr;
    size_t n = 0;
};

inline int dev_alloc(EngineHost *e, DevBuf &b, size_t n) {  // grows only
    if (b.p && b.n >= n) return 0;
    if (b.p) HIPCHECK(e, hipFree(b.p));
    b.p = nullptr;
    b.n = 0;
    HIPCHECK(e, hipMalloc(reinterpret_cast<void **>(&b.p), (n ? n : 1) * sizeof(float)));
    b.n = n;
    return 0;
}

inline int dev_upload(EngineHost *e, DevBuf &b, const std::vector<float> &h) {
    int rc = dev_alloc(e, b, h.size());
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(b.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

inline void dev_free(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
}

inline uint16_t f16_rne(float x) {  // IEEE half, round to nearest even (the host compiler's _Float16 conversion)
    const _Float16 h = (_Float16)x;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// operand planes per precision mode: 0 -> 3 bf16 planes (hi, mid, lo; six products), 1 -> 1 fp16 plane, 2 -> 2 bf16 planes
// (hi, mid; three products hi*hi + hi*mid + mid*hi)
inline int operand_planes(int precision) { return precision == 1 ? 1 : (precision == 2 ? 2 : 3); }

// The plane count is a property of the BUFFER, not only of the precision mode: with the fp16 pair format on (split_f16pair.h; precision
// 0 only, decided when the weights are loaded) the buffers of kind kGemmA hold two fp16 planes.  kFeature: the STFT features and what
// reads them (xinP[0]) - the magnitude channel scales with the input level, so they stay on bf16 planes; kConvAct: the activation
// planes of the convolution / skip path (xinP[i >= 1], decinP, decP), bounded by a norm or by the skip gate's convex combination;
// kGemmA: the A operands of the bottleneck GEMMs and of the recurrence (gruinP, seqP), bounded by a norm and by the GRU cell.
// conv_on = false (SE_F16_PAIR_CONV=0): the convolution path keeps its bf16 planes while the bottleneck runs the pair.
enum class PlaneBuf { kFeature, kConvAct, kGemmA };
inline PlaneFmt buffer_format(int precision, bool pair_on, PlaneBuf kind, bool conv_on = true) {
    const bool takes = kind == PlaneBuf::kGemmA || (kind == PlaneBuf::kConvAct && conv_on);
    return pair_on && precision == 0 && takes ? PlaneFmt::kF16Pair : PlaneFmt::kBf16;
}
inline int buffer_planes(int precision, bool pair_on, PlaneBuf kind, bool conv_on = true) {
    return buffer_format(precision, pair_on, kind, conv_on) == PlaneFmt::kF16Pair ? kPairPlanesA : operand_planes(precision);
}
// The ORDER of the planes is a property of the buffer too: the kGemmA buffers and the weights k_gemm_p multiplies them with are K-blocked
// ([row][K / 32][plane][32], gemm_kblock.h) where the pair is on with its two stored weight planes (wpl = the stored weight planes of the
// pair) and the knob (SE_GEMM_KBLOCK) allows it.  Everything else is plane-major [plane][row][K].
inline bool buffer_kblocked(int precision, bool pair_on, int wpl, bool knob, PlaneBuf kind) {
    return knob && kind == PlaneBuf::kGemmA && wpl == kPairPlanesW2 && buffer_format(precision, pair_on, kind) == PlaneFmt::kF16Pair;
}

// the fp16-pair planes (2^11 hi, lo, hi) of a [rows][cols] fp32 matrix -> device buffer of 3*rows*cols uint16 (the shape of upload_planes);
// wpl = kPairPlanesW2: the two stored planes (lo, hi), 2*rows*cols uint16; kblock_cols > 0 (two stored planes only): K-blocked rows of
// that many columns (gemm_kblock.h)
inline int upload_planes_pair(EngineHost *e, DevBuf &b, const std::vector<float> &w, int wpl = kPairPlanesW, size_t kblock_cols = 0) {
    std::vector<uint16_t> planes((size_t)wpl * w.size());
    if (wpl == kPairPlanesW2 && kblock_cols) pair_weight_matrix2_kblock(w.data(), w.size() / kblock_cols, kblock_cols, planes.data());
    else if (wpl == kPairPlanesW2) pair_weight_matrix2(w.data(), w.size(), planes.data());
    else pair_weight_matrix(w.data(), w.size(), planes.data());
    int rc = dev_alloc(e, b, (planes.size() + 1) / 2);
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(b.p, planes.data(), planes.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return 0;
}

// the operand planes of a [rows][cols] fp32 matrix at `precision` -> device buffer of PL*rows*cols uint16
inline int upload_planes(EngineHost *e, DevBuf &b, const std::vector<float> &w, int precision) {
    const size_t n = w.size();
    const int PL = operand_planes(precision);
    std::vector<uint16_t> planes(PL * n);
    for (size_t i = 0; i < n; i++) {
        const float x = w[i];
        if (precision == 1) { planes[i] = f16_rne(x); continue; }
        const uint16_t h = bf16_rne(x);
        const float r1 = x - bf16_to_f32(h);
        const uint16_t m = bf16_rne(r1);
        planes[i] = h; planes[n + i] = m;
        if (PL > 2) planes[2 * n + i] = bf16_rne(r1 - bf16_to_f32(m));
    }
    int rc = dev_alloc(e, b, (PL * n + 1) / 2);
    if (rc) return rc;
    HIPCHECK(e, hipMemcpy(b.p, planes.data(), planes.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return 0;
}

inline const std::vector<float> *param(EngineHost *e, const std::string &key, size_t expect) {
    auto it = e->params.find(key);
    if (it == e->params.end()) {
        fail(e, SE_ERR_PARAM_MISSING, "parameter %s was never loaded", key.c_str());
        return nullptr;
    }
    if (it->second.size() != expect) {
        fail(e, SE_ERR_SHAPE, "parameter %s has %zu elements, expected %zu", key.c_str(), it->second.size(), expect);
        return nullptr;
    }
    return &it->second;
}

// the tail of *_load_param: the host copy of an accepted key
inline int store_param(EngineHost *e, const std::string &key, const float *host_data, const int64_t *shape, int ndim) {
    size_t cnt = 1;
    for (int i = 0; i < ndim; i++) {
        if (shape[i] < 0) return fail(e, SE_ERR_SHAPE, "negative dimension in %s", key.c_str());
        cnt *= (size_t)shape[i];
    }
    e->params[key].assign(host_data, host_data + cnt);
    return SE_OK;
}

// A chains call's plan on the device: plan_dev (8 * B floats of the engine's own) gets the staging vector in one copy, and the plan's
// device pointers are carved out of it.  Synchronises `st`: the staging vector and the caller's host arrays live for the call only.
inline int upload_plan(EngineHost *e, DevBuf &plan_dev, ChainPlan &plan, hipStream_t st) {
    int rc = dev_alloc(e, plan_dev, plan.staging_floats());
    if (rc) return rc;
    HIPCHECK(e, hipMemcpyAsync(plan_dev.p, plan.staging.data(), plan.staging.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIPCHECK(e, hipStreamSynchronize(st));
    plan.carve(plan_dev.p);
    return 0;
}

}  // namespace se
