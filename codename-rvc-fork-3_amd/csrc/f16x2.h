// Primitives of the error-corrected fp16 PAIR (Ootomo & Yokota, "Recovering single precision accuracy from Tensor Cores while
// surpassing the FP32 theoretical peak performance", 2022): an fp32 value v travels as
//     hi = fp16(v),   lo = fp16((v - hi) * 2^11)                    (both round to nearest even; v - hi is exact in fp32)
// and a product is  w x ~= w_hi x_hi + 2^-11 (w_hi x_lo + w_lo x_hi);  the dropped w_lo x_lo is <= 2^-22 |w x|.
// The 2^11 keeps lo a NORMAL fp16 wherever hi is one (|v - hi| <= 2^-11 |hi| would otherwise sit 11 binades nearer the subnormals).
// Range: |v| <= 65504 (above it hi is inf).  Below |v| ~ 2^-14 hi is an fp16 subnormal: the pair then still holds v to
// 2^-25 / 2^11 absolute, as long as subnormal operands are not flushed (convbf1.hip says what the hardware does).
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include "bf16x3.h"

namespace rvc {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float F16_MAX = 65504.f;
constexpr float F16X2_LO_SCALE = 2048.f;             // 2^11
constexpr float F16X2_LO_UNSCALE = 1.f / 2048.f;

// (a, b), each clamped to +-65504 (a NaN comes out as -65504), -> hi = two fp16 (a in the low half), lo = the two scaled rests;
// non-packed fp32 operations (bf16x3.h: these run next to another wave's matrix instructions)
__device__ __forceinline__ void split_f16x2_np(float a, float b, unsigned &hi, unsigned &lo) {
    a = __builtin_fminf(__builtin_fmaxf(a, -F16_MAX), F16_MAX);
    b = __builtin_fminf(__builtin_fmaxf(b, -F16_MAX), F16_MAX);
    const _Float16 ah = (_Float16)a, bh = (_Float16)b;                      // v_cvt_f16_f32: round to nearest even, subnormals kept
    hi = __builtin_bit_cast(unsigned, f16x2{ah, bh});
    const float ar = mul_np(sub_np(a, (float)ah), F16X2_LO_SCALE), br = mul_np(sub_np(b, (float)bh), F16X2_LO_SCALE);
    lo = __builtin_bit_cast(unsigned, f16x2{(_Float16)ar, (_Float16)br});
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// fp32 -> fp16 bits, round to nearest even, subnormals kept, overflow to inf (what v_cvt_f16_f32 and torch's .half() do)
static inline uint16_t f16_rne_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // >= 65520: rounds to inf
    if (u < 0x38800000u) {                                                  // below 2^-14: a subnormal (or zero), quantum 2^-24
        if (u < 0x33000000u) return sign;                                   // below 2^-25: zero (2^-25 itself ties to even = zero)
        const int e = (int)(u >> 23);                                       // biased exponent, 102 .. 112
        const uint32_t m = (u & 0x7fffffu) | 0x800000u;                     // 24-bit significand: v = m 2^(e - 150)
        const int sh = 126 - e;                                             // v / 2^-24 = m >> sh, sh 14 .. 24
        const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), halfway = 1u << (sh - 1);
        return (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = u + 0xfffu + ((u >> 13) & 1u);                       // round the 13 dropped bits to nearest even
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}
static inline float f16_bits_to_float_host(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 31) {
        u = sign | 0x7f800000u | (m << 13);
    } else if (e == 0) {
        float f = (float)m * 5.9604644775390625e-8f;                        // m 2^-24, exact
        memcpy(&u, &f, 4);
        u |= sign;
    } else {
        u = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// v (finite, |v| <= 65504) -> (hi, lo) as above
static inline void f16x2_split_host(float v, uint16_t *hi, uint16_t *lo) {
    *hi = f16_rne_host(v);
    *lo = f16_rne_host((v - f16_bits_to_float_host(*hi)) * F16X2_LO_SCALE);
}

}  // namespace rvc
