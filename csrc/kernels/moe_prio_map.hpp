// The order of the per-expert top-S select (K15): the key of a gate weight, the 64-bit word of an
// assignment and the step of the MSD radix select over those words.  Plain C++ (no HIP types), the
// same code on the host and on the device: csrc/kernels/test_moe_prio_map.cpp runs the whole select
// on the CPU against std::sort.  k_moe_prio_keys / _select / _mask take their order from here only.
//
//   key(bits)   unsigned order == float order of the float with these bits, -0 folded onto +0 (the
//               map of gate_key in moe_gate_common.hpp, on the bits so that the host can run it);
//               defined for every pattern: a positive NaN sorts above +inf, a negative one below -inf
//   word(p, a)  key(p) << 32 | (0xffffffff - a): a larger word is a higher priority, and among equal
//               priorities the lower assignment index a; words of distinct assignments are distinct
//   select      the L-th largest of a set of words, 1 <= L <= size, by 8 passes over 8-bit digits from
//               the top: a pass counts digit(w, pass) of every word that still matches the prefix
//               (candidate), digit_step picks the digit that holds the L-th largest and what is left
//               of L inside it.  After kPasses passes the prefix is that word itself.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_PRIO_HD __host__ __device__ inline
#else
#define MP4X_PRIO_HD inline
#endif

namespace mp4x {
namespace prio {

constexpr int kBins = 256;
constexpr int kPasses = 8;

MP4X_PRIO_HD uint32_t key(uint32_t bits) {
  if ((bits << 1) == 0) bits = 0;
  return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

MP4X_PRIO_HD uint64_t word(uint32_t priority_bits, uint32_t a) {
  return ((uint64_t)key(priority_bits) << 32) | (uint64_t)(0xffffffffu - a);
}

// The digit of pass 0 is the top byte.
MP4X_PRIO_HD int digit(uint64_t w, int pass) { return (int)((w >> (8 * (kPasses - 1 - pass))) & 0xffu); }

// Does w carry the `pass` digits chosen so far (the low `pass` bytes of prefix)?  Pass 0: every word.
MP4X_PRIO_HD bool candidate(uint64_t w, uint64_t prefix, int pass) {
  return pass == 0 || (w >> (8 * (kPasses - pass))) == prefix;
}

// hist[d] = candidates with digit d; `remaining` = L inside the candidates, 1 <= remaining <= their
// number.  Returns the digit d that holds the remaining-th largest candidate and leaves in
// `remaining` its rank among the candidates with that digit (again 1 <= remaining <= hist[d]).
// A histogram that breaks the precondition gives digit 0 and remaining clamped to >= 1: no trip
// count depends on the data.
MP4X_PRIO_HD int digit_step(const uint32_t* hist, uint64_t* remaining) {
  uint64_t r = *remaining;
  for (int d = kBins - 1; d > 0; --d) {
    const uint64_t h = hist[d];
    if (h >= r) {
      *remaining = r;
      return d;
    }
    r -= h;
  }
  *remaining = r < 1 ? 1 : r;
  return 0;
}

// What the mask does with an expert: kAll when it holds no more than its limit (no selection
// work), kNone for a limit of 0, else kSelect with the limit-th largest word as threshold.
enum : int { kAll = 0, kSelect = 1, kNone = 2 };

MP4X_PRIO_HD int mode(int64_t cnt, int64_t limit) { return cnt <= limit ? kAll : (limit <= 0 ? kNone : kSelect); }

MP4X_PRIO_HD bool keeps(int m, uint64_t tau, uint64_t w) { return m == kAll || (m == kSelect && w >= tau); }

}  // namespace prio
}  // namespace mp4x
