// fp32 <-> 16-bit conversions of the weight packers (round-to-nearest-even), in integer arithmetic so that the host and the device produce the same
// bits by construction: one copy, compiled for both sides.  weight_layout.h builds the layouts on it in the same way: one interpreter of a piece, which
// pack.hip's kernels and engine.cpp's host packers both loop over.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldx {

__host__ __device__ inline uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__host__ __device__ inline float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

__host__ __device__ inline float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16;
    uint32_t exp = (h >> 10) & 0x1f, man = h & 0x3ff, out;
    if (exp == 0) {
        if (man == 0) out = sign;
        else {
            exp = 127 - 15 + 1;
            while (!(man & 0x400)) { man <<= 1; --exp; }
            man &= 0x3ff;
            out = sign | (exp << 23) | (man << 13);
        }
    } else if (exp == 31) out = sign | 0x7f800000u | (man << 13);
    else out = sign | ((exp + 127 - 15) << 23) | (man << 13);
    return bits_f32(out);
}
__host__ __device__ inline uint16_t float_to_half(float f) {
    uint32_t x = f32_bits(f);
    const uint32_t sign = (x >> 16) & 0x8000;
    x &= 0x7fffffff;
    if (x >= 0x7f800000) return (uint16_t)(sign | 0x7c00 | ((x > 0x7f800000) ? 0x200 : 0));
    if (x >= 0x477ff000) return (uint16_t)(sign | 0x7c00);                       // overflow -> inf
    if (x < 0x33000001) return (uint16_t)sign;                                  // underflow -> 0
    int exp = (int)(x >> 23) - 127 + 15;
    uint32_t man = x & 0x7fffff;
    if (exp <= 0) {                                                              // subnormal
        man |= 0x800000;
        const int shift = 14 - exp;
        uint32_t hm = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1), halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (hm & 1))) ++hm;
        return (uint16_t)(sign | hm);
    }
    uint32_t hm = man >> 13;
    const uint32_t rem = man & 0x1fff;
    uint32_t out = ((uint32_t)exp << 10) | hm;
    if (rem > 0x1000 || (rem == 0x1000 && (hm & 1))) ++out;
    return (uint16_t)(sign | out);
}
__host__ __device__ inline float bf16_to_float(uint16_t h) { return bits_f32((uint32_t)h << 16); }
__host__ __device__ inline uint16_t float_to_bf16(float f) {
    uint32_t x = f32_bits(f);
    if ((x & 0x7fffffff) > 0x7f800000) return (uint16_t)((x >> 16) | 0x40);
    x += 0x7fff + ((x >> 16) & 1);
    return (uint16_t)(x >> 16);
}

// GGML Q8_0: blocks of an fp16 scale d and 32 int8 values q.  A weight is fp16_rne(float(d) * q): the product (11 x 8 significant bits) is exact in
// fp32, so this is torch's fp16 d * q with its single rounding, NaN, overflow to inf, subnormals and -0 included.
constexpr int Q8_0_BLOCK = 32, Q8_0_BYTES = 34;
__host__ __device__ inline uint16_t q8_0_value(uint16_t d, int8_t q) { return float_to_half(half_to_float(d) * (float)q); }

}  // namespace ldx
