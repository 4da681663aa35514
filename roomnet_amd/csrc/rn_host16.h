// The 16-bit storage types on the host: plain C++ (no HIP), shared by the library's translation units (through rn_internal.h) and
// by the weight packers of rn_pack.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "roomnet_hip.h"

// ---- the 16-bit storage types on the host: round to nearest even, and back
inline unsigned short f32_to_bf16(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<unsigned short>((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<unsigned short>(u >> 16);
}

inline unsigned short f32_to_f16(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return static_cast<unsigned short>(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));
    if (x >= 0x477ff000u) return static_cast<unsigned short>(sign | 0x7c00u);          // overflow -> inf
    if (x < 0x33000001u) return static_cast<unsigned short>(sign);                     // underflow -> 0
    int e = static_cast<int>(x >> 23) - 127;
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    int shift;
    if (e < -14) {
        shift = 13 + (-14 - e);
        e = -15;
    } else {
        shift = 13;
    }
    uint32_t half = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (half & 1))) ++half;
    uint32_t out;
    if (e == -15)
        out = half;                                   // subnormal (may carry into exponent 1)
    else
        out = (static_cast<uint32_t>(e + 15) << 10) + (half - 0x400u);
    return static_cast<unsigned short>(sign | out);
}

inline float bf16_bits_to_f32(unsigned short u) {
    const unsigned bits = static_cast<unsigned>(u) << 16;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

inline float f16_to_f32(unsigned short h) {
    const uint32_t sign = static_cast<uint32_t>(h & 0x8000u) << 16;
    const int e = (h >> 10) & 0x1f;
    const uint32_t m = h & 0x3ffu;
    float mag;
    if (e == 0)
        mag = std::ldexp(static_cast<float>(m), -24);                    // zero / subnormal
    else if (e == 31)
        mag = m ? std::nanf("") : INFINITY;
    else
        mag = std::ldexp(static_cast<float>(m | 0x400u), e - 25);
    uint32_t u;
    std::memcpy(&u, &mag, 4);
    u |= sign;
    std::memcpy(&mag, &u, 4);
    return mag;
}

// a handle's storage type (RN_DTYPE_BF16 / RN_DTYPE_F16)
inline unsigned short rn_to16(float v, int dtype) { return dtype == RN_DTYPE_BF16 ? f32_to_bf16(v) : f32_to_f16(v); }
inline float rn_from16(unsigned short u, int dtype) { return dtype == RN_DTYPE_BF16 ? bf16_bits_to_f32(u) : f16_to_f32(u); }
