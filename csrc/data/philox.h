// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC 2011), the counter-based generator of Random123, in plain C++
// for the host and the device: a pure function of a 128-bit counter and a
// 64-bit key, no state.  Known answers (counter, key -> output), all hex:
//   (0, 0, 0, 0), (0, 0)                                -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   all ones, all ones                                  -> 408f276d 41c83b0e a20bc7c6 6d5451fd
//   243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMP_PHILOX_HD __host__ __device__ inline
#else
#define DMP_PHILOX_HD inline
#endif

namespace dmp {

struct Philox4 {
  uint32_t v[4];
};

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;  // round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;  // Weyl key increments

DMP_PHILOX_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // 32 x 32 -> 64-bit products in unsigned arithmetic: high and low words
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// 23 random bits -> a uniform in (0, 1): (2 m + 1) / 2^24 with m = r >> 9, an odd
// multiple of 2^-24 below 1: exact in fp32, never 0 or 1.
DMP_PHILOX_HD float philox_uniform(uint32_t r) { return (float)(2u * (r >> 9) + 1u) * 0x1p-24f; }

}  // namespace dmp
