// split_f16pair.h - the "fp16 pair" operand format of the fp32-accurate mode (precision 0), next to the three bf16 planes of split_bf16.h.
//
// An fp32 value x is carried as two fp16 numbers
//     hi = fp16(x)            lo = fp16((x - hi) * 2^11)            x ~= hi + lo * 2^-11   (to 2^-23 relative, 2^-36 absolute)
// x - hi is exact in fp32 and has at most 13 significant bits; the scale keeps lo in the exponent range of x, so lo is a normal fp16
// number wherever hi is (an unscaled lo falls into fp16 subnormals for |x| < 2^-3 and loses its bits there).  |x| is clamped to the
// largest finite fp16 first: an out-of-range operand becomes a clipped finite value, never inf or NaN.
// A product needs three matrix-core terms, a_hi b_hi + 2^-11 (a_hi b_lo + a_lo b_hi); the dropped a_lo b_lo is <= 2^-24 relative.  The
// weight side stores its three planes as (2^11 w_hi, w_lo, w_hi) - w_lo being the stored, scaled low part - so that
//     a_hi W0 + a_hi W1 + a_lo W2 = 2^11 (a w)
// accumulates in ONE fp32 accumulator set and the epilogue multiplies by 2^-11 (exact) ahead of the bias.  2^11 w_hi is finite for
// |w| < 2^4, which the engine checks when the weights are loaded (se_engine.hip: f16_pair_guard).
// The host half is plain C++ (no HIP): the engine's weight preparation and tests/f16_pair_check.cpp compile the same code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SE_PAIR_HD __host__ __device__
#else
#define SE_PAIR_HD
#endif

namespace se {

// what the planes of an operand buffer hold.  kBf16: PL bf16 planes that sum to x (PL = 1: one fp16 plane); kF16Pair: (hi, lo) above
enum class PlaneFmt : int { kBf16 = 0, kF16Pair = 1 };

constexpr float kPairScale = 2048.0f, kPairInvScale = 1.0f / 2048.0f, kPairMax = 65504.0f;
constexpr int kPairPlanesA = 2, kPairPlanesW = 3;  // planes of an activation / a weight operand

// IEEE binary16 <-> fp32 on the bits, round to nearest even, subnormals kept (what v_cvt_f16_f32 / v_cvt_f32_f16 do on the device)
SE_PAIR_HD inline uint16_t pair_f16_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)x;
    return __builtin_bit_cast(uint16_t, h);
#else
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);   // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to inf
    if (u < 0x38800000u) {                                    // below 2^-14: subnormal fp16, a multiple of 2^-24
        if (u < 0x33000000u) return sign;                     // < 2^-25 -> 0 (2^-25 itself ties to even = 0, handled below)
        const int e = (int)(u >> 23);                         // biased fp32 exponent, 102 .. 112
        const uint32_t m = (u & 0x7fffffu) | 0x800000u;       // 24-bit significand
        const int sh = 126 - e;                               // value = m * 2^(e - 150); units of 2^-24: m >> (126 - e)
        const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), halfway = 1u << (sh - 1);
        return (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = u + 0xfffu + ((u >> 13) & 1u);         // round the 13 dropped bits to nearest even
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
#endif
}

SE_PAIR_HD inline float pair_f16_value(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, h);
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 31u) u = sign | 0x7f800000u | (m << 13);
    else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
    else {
        float f = (float)m * 5.9604644775390625e-8f;  // m * 2^-24, exact
        memcpy(&u, &f, 4);
        u |= sign;
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// x -> (hi, lo) as fp16 bit patterns
SE_PAIR_HD inline void split2h(float x, uint16_t &hi, uint16_t &lo) {
    x = x < -kPairMax ? -kPairMax : (x > kPairMax ? kPairMax : x);  // (a NaN passes both comparisons: cleared below)
    if (x != x) x = 0.0f;
    hi = pair_f16_bits(x);
    lo = pair_f16_bits((x - pair_f16_value(hi)) * kPairScale);
    // Canonical form.  A low part within 2^-12 of half an ulp of hi rounds UP to that half ulp, which puts the stored value hi + lo 2^-11
    // (exact in fp32: 23 bits) on a tie of the fp16 grid, where an odd hi is not what fp16() of the stored value returns.  The pair is
    // then re-formed from the stored value - the same value, the other representation - so that split2h(join2h(hi, lo)) == (hi, lo) for
    // every pair this function returns: a history that goes through export_state / import_state comes back with the same bits.
    const float stored = pair_f16_value(hi) + pair_f16_value(lo) * kPairInvScale;
    const uint16_t hi2 = pair_f16_bits(stored);
    if (hi2 != hi) {
        hi = hi2;
        lo = pair_f16_bits((stored - pair_f16_value(hi2)) * kPairScale);  // (+- half an ulp of hi2: exact)
    }
    if ((lo & 0x7fffu) == 0) lo = 0;  // (a negative residual below 2^-25 rounds to -0: the stored zero is +0)
}

// the inverse, one fp32 add (the product is exact): the same expression in the device readers and the host taps
SE_PAIR_HD inline float join2h(uint16_t hi, uint16_t lo) { return pair_f16_value(hi) + pair_f16_value(lo) * kPairInvScale; }

// the three weight planes (2^11 w_hi, w_lo, w_hi); 2^11 w_hi is exact (and finite for |w| < 2^4)
inline void pair_weight_planes(float w, uint16_t (&p)[3]) {
    uint16_t hi, lo;
    split2h(w, hi, lo);
    p[0] = pair_f16_bits(pair_f16_value(hi) * kPairScale);
    p[1] = lo;
    p[2] = hi;
}

// a [rows][cols] weight matrix as planes [3][rows][cols] (the layout of engine_host.h: upload_planes)
inline void pair_weight_matrix(const float *w, size_t n, uint16_t *planes) {
    for (size_t i = 0; i < n; i++) {
        uint16_t p[3];
        pair_weight_planes(w[i], p);
        planes[i] = p[0]; planes[n + i] = p[1]; planes[2 * n + i] = p[2];
    }
}

// ---- two STORED weight planes (w_lo, w_hi) ----
// Plane 0 of the three is 2^11 times plane 2, exact in fp16 wherever it is finite (|w| < 2^4: the guard), subnormals and zeros
// included.  The kernels' two-plane instances (weight-plane parameter 2) fetch (w_lo, w_hi) and form 2^11 w_hi in registers with one
// packed fp16 multiply per dword (pair_scale_hi below): the same operand bits into the same MFMAs, a third fewer weight bytes.
constexpr int kPairPlanesW2 = 2;

// (w_lo, w_hi): planes 1 and 2 of pair_weight_planes
inline void pair_weight_planes2(float w, uint16_t (&p)[2]) {
    uint16_t q[3];
    pair_weight_planes(w, q);
    p[0] = q[1];
    p[1] = q[2];
}

// `parts` of conv_weight_image.h for either stored plane count (slots past `planes` are left alone)
inline void pair_weight_parts(float w, int planes, uint16_t (&p)[3]) {
    uint16_t q[3];
    pair_weight_planes(w, q);
    if (planes == kPairPlanesW2) { p[0] = q[1]; p[1] = q[2]; }
    else { p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
}

// a [rows][cols] weight matrix as planes [2][rows][cols] = (w_lo, w_hi)
inline void pair_weight_matrix2(const float *w, size_t n, uint16_t *planes) {
    for (size_t i = 0; i < n; i++) {
        uint16_t p[2];
        pair_weight_planes2(w[i], p);
        planes[i] = p[0]; planes[n + i] = p[1];
    }
}

// what the device does to one stored w_hi: ONE fp16 multiply by 2^11 (round to nearest even, subnormals kept).  Host form for the
// tests; the product is exact, so the fp32 route through pair_f16_bits gives the same bits.
inline uint16_t pair_scale_hi_bits(uint16_t hi) { return pair_f16_bits(pair_f16_value(hi) * kPairScale); }

#if defined(__HIPCC__)
// 2^11 w_hi from a w_hi fragment (8 fp16 in four dwords): four v_pk_mul_f16.  A multiply, not an exponent add: zeros and
// subnormals come out right.
template <class V4 /* four dwords: uint4 or an ext_vector of 4 unsigned */>
__device__ __forceinline__ V4 pair_scale_hi(const V4 &hi) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    static_assert(sizeof(V4) == 16, "one 16-byte fragment");
    const h8 v = __builtin_bit_cast(h8, hi) * (_Float16)2048.0f;
    return __builtin_bit_cast(V4, v);
}

// fp32 x 8 -> the two planes of one 16-byte piece (8 channels): the pair flavour of split_store8 (conv_p.hip.h)
__device__ __forceinline__ void split_store8_pair(const float (&v)[8], uint4 *dst, long plane_stride) {
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
    u16x8 h, l;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        uint16_t hh, ll;
        split2h(v[c], hh, ll);
        h[c] = hh; l[c] = ll;
    }
    dst[0] = __builtin_bit_cast(uint4, h);
    dst[plane_stride] = __builtin_bit_cast(uint4, l);
}
#endif

}  // namespace se
