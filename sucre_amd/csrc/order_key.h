// The order-preserving integer image of a float32 bit pattern, shared by the radix selects (plot.hip: one image,
// pool.hip: a pool of images).
#pragma once
#include <hip/hip_runtime.h>

namespace sucre {

__device__ __forceinline__ uint32_t order_key(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone: a < b  <=>  key(a) < key(b)
}

__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

}  // namespace sucre
