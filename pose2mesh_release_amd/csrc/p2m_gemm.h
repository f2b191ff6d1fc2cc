// What more than one translation unit of the dense contractions needs (gemm_planes.hip, gemm_tn.hip, weights.hip, amax.hip):
// the block tile, the layout of a pre-split weight image, and the host-side launch helpers.
#pragma once
#include <type_traits>

#include "p2m_split.h"

namespace p2m {

constexpr int BM = 128;
constexpr int BK = 32;

static inline int slices_of(int arith) { return arith == P2M_ARITH_F16X2 ? 2 : 3; }
// the amax word of a two-fp16-slice weight image trails its slices (8 elements = 16 bytes: keeps images 16-byte sized)
static inline const unsigned* weight_amax_word(const void* Bx, int arith, long Npad, long K) {
  return arith == P2M_ARITH_F16X2
             ? reinterpret_cast<const unsigned*>(static_cast<const unsigned short*>(Bx) + 2 * Npad * K)
             : nullptr;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// *word = max |x[i]|, i < n, by one block (k_amax_one_block, amax.hip): the amax word of a small tensor, no zeroing before
void amax_one_block(const float* x, long n, unsigned* word, hipStream_t stream);

// Runtime flags -> template arguments: f(t0, t1, ..) with ti std::true_type or std::false_type as flag i is set or not, so
// that a launch names its instantiation by `decltype(ti)::value` instead of an if / else ladder per flag.
template <class F>
static inline void with_bools(F&& f) { f(); }
template <class F, class... Rest>
static inline void with_bools(F&& f, bool flag, Rest... rest) {
  if (flag) with_bools([&](auto... t) { f(std::true_type{}, t...); }, rest...);
  else with_bools([&](auto... t) { f(std::false_type{}, t...); }, rest...);
}

}  // namespace p2m
