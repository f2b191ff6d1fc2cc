// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain C++, for host
// and device alike: the one counter-based stream of the sample-noise kernels (csrc/sample.hip).  tests/sample_ref.py restates
// it in numpy.  Known answers: counter 0,0,0,0 key 0,0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; counter 243f6a88 85a308d3
// 13198a2e 03707344 key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define P2M_PHILOX_FN __host__ __device__ __forceinline__
#else
#define P2M_PHILOX_FN inline
#endif

namespace p2m {

struct Philox4 {
  uint32_t w[4];
};

P2M_PHILOX_FN Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The stream of include/p2m.h ("training-sample noise"): key = seed, counter = (global sample index, joint | stage << 8,
// draw block).
P2M_PHILOX_FN Philox4 philox_draw(uint64_t seed, uint64_t index, uint32_t joint, uint32_t stage, uint32_t block) {
  return philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), joint | (stage << 8), block, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// A uniform in [0, 1) with 24 bits: exact in fp32 and fp64 alike.
P2M_PHILOX_FN float philox_uniform(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

}  // namespace p2m
