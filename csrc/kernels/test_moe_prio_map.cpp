// Stand-alone CPU test of csrc/kernels/moe_prio_map.hpp (build with -fsanitize=address,undefined):
// the key's order against the float order, the word's tie rule, and the whole 8-pass select, run
// exactly as k_moe_prio_select runs it (histogram of the candidates' digit, digit_step, prefix),
// against std::sort for every limit of small segments and for sampled limits of large ones, over
// priorities chosen to make the passes hard: constants (only the index bytes decide), last-bit
// neighbours, +-0, +-inf, both NaNs, denormals, and indices that reach the third index byte.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "moe_prio_map.hpp"

using namespace mp4x;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (++failures < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                   \
  } while (0)

static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float float_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

// The select as the kernel runs it; returns the L-th largest word (1 <= L <= size).
static uint64_t radix_select(const std::vector<uint64_t>& seg, uint64_t L) {
  uint64_t prefix = 0, remaining = L;
  for (int pass = 0; pass < prio::kPasses; ++pass) {
    uint32_t hist[prio::kBins] = {0};
    uint64_t cand = 0;
    for (uint64_t w : seg)
      if (prio::candidate(w, prefix, pass)) {
        ++hist[prio::digit(w, pass)];
        ++cand;
      }
    CHECK(remaining >= 1 && remaining <= cand);
    const int d = prio::digit_step(hist, &remaining);
    CHECK(d >= 0 && d < prio::kBins);
    CHECK(remaining >= 1 && remaining <= hist[d]);
    prefix = (prefix << 8) | (uint64_t)d;
  }
  CHECK(remaining == 1);             // words are distinct: one candidate is left
  return prefix;
}

static void check_segment(const std::vector<uint32_t>& pbits, const std::vector<uint32_t>& idx, bool every_limit) {
  std::vector<uint64_t> seg(pbits.size());
  for (size_t i = 0; i < seg.size(); ++i) seg[i] = prio::word(pbits[i], idx[i]);
  std::vector<uint64_t> sorted(seg);
  std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
  for (size_t i = 1; i < sorted.size(); ++i) CHECK(sorted[i - 1] != sorted[i]);
  const size_t n = seg.size();
  std::vector<uint64_t> limits;
  if (every_limit) {
    for (uint64_t L = 1; L <= n; ++L) limits.push_back(L);
  } else {
    limits = {1, 2, n / 3 + 1, n / 2, n - 1, n};
    for (int i = 0; i < 6; ++i) limits.push_back(1 + rnd() % n);
  }
  for (uint64_t L : limits) {
    if (L < 1 || L > n) continue;
    const uint64_t tau = radix_select(seg, L);
    CHECK(tau == sorted[L - 1]);
    uint64_t kept = 0;
    for (uint64_t w : seg) kept += prio::keeps(prio::kSelect, tau, w);
    CHECK(kept == L);
  }
}

int main() {
  // ---- the key: unsigned order == float order, -0 == +0, NaNs outside the infinities
  const float inf = INFINITY;
  std::vector<uint32_t> special = {bits_of(0.0f), bits_of(-0.0f), bits_of(inf), bits_of(-inf), 0x7fc00000u, 0xffc00000u,
                                   0x7fffffffu, 0xffffffffu, 0x7f800001u, 0xff800001u, 0x00000001u, 0x80000001u,
                                   0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u, bits_of(1.0f), bits_of(-1.0f),
                                   0x3f800001u, 0x3f7fffffu, bits_of(0.5f), bits_of(3.0e38f), bits_of(-3.0e38f)};
  std::vector<uint32_t> pool(special);
  for (int i = 0; i < 2000; ++i) pool.push_back(rnd());
  for (size_t i = 0; i < pool.size(); ++i) {
    for (size_t j = 0; j < (i < special.size() ? pool.size() : special.size()); ++j) {
      const float a = float_of(pool[i]), b = float_of(pool[j]);
      const uint32_t ka = prio::key(pool[i]), kb = prio::key(pool[j]);
      if (!std::isnan(a) && !std::isnan(b)) {
        CHECK((a < b) == (ka < kb));
        CHECK((a == b) == (ka == kb));
      }
      if (std::isnan(a) && !std::isnan(b)) CHECK((pool[i] >> 31) ? ka < kb : ka > kb);
    }
  }
  CHECK(prio::key(bits_of(-0.0f)) == prio::key(bits_of(0.0f)));
  CHECK(prio::key(0x7fc00000u) > prio::key(bits_of(inf)));
  CHECK(prio::key(0xffc00000u) < prio::key(bits_of(-inf)));
  // ---- the word: the priority first, then the lower index; the largest word is all ones
  CHECK(prio::word(bits_of(1.0f), 7) > prio::word(bits_of(0.5f), 3));
  CHECK(prio::word(bits_of(1.0f), 3) > prio::word(bits_of(1.0f), 7));
  CHECK(prio::word(bits_of(0.0f), 3) > prio::word(bits_of(-0.0f), 7));
  CHECK(prio::word(0x7fffffffu, 0) == ~0ull);
  CHECK(prio::digit(0x0123456789abcdefull, 0) == 0x01 && prio::digit(0x0123456789abcdefull, 7) == 0xef);
  CHECK(prio::candidate(0x0123456789abcdefull, 0, 0) && prio::candidate(0x0123456789abcdefull, 0x0123, 2) &&
        !prio::candidate(0x0123456789abcdefull, 0x0124, 2) && prio::candidate(0x0123456789abcdefull, 0x0123456789abcdull, 7));
  // ---- the modes
  CHECK(prio::mode(5, 5) == prio::kAll && prio::mode(5, 6) == prio::kAll && prio::mode(0, 0) == prio::kAll);
  CHECK(prio::mode(5, 0) == prio::kNone && prio::mode(5, -3) == prio::kNone && prio::mode(0, -1) == prio::kNone);
  CHECK(prio::mode(5, 4) == prio::kSelect && prio::mode(5, 1) == prio::kSelect);
  CHECK(prio::keeps(prio::kAll, 0, 0) && !prio::keeps(prio::kNone, 0, ~0ull) && prio::keeps(prio::kSelect, 5, 5) &&
        !prio::keeps(prio::kSelect, 5, 4));
  // ---- a histogram that breaks the precondition: a digit in range, remaining >= 1, no loop past the bins
  {
    uint32_t hist[prio::kBins] = {0};
    uint64_t r = 9;
    const int d = prio::digit_step(hist, &r);
    CHECK(d == 0 && r >= 1);
    r = 2;
    hist[200] = 3;
    CHECK(prio::digit_step(hist, &r) == 200 && r == 2);
  }
  // ---- the select, every limit, small segments
  for (int trial = 0; trial < 60; ++trial) {
    const size_t n = 1 + rnd() % 300;
    std::vector<uint32_t> p(n), idx(n);
    const int kind = trial % 6;
    uint32_t a = rnd() % 1000;
    for (size_t i = 0; i < n; ++i) {
      a += 1 + rnd() % 5;            // ascending, distinct indices, as a segment's are
      idx[i] = a;
      switch (kind) {
        case 0: p[i] = bits_of(0.25f); break;                                  // constant: the index decides
        case 1: p[i] = 0x3f000000u + (rnd() & 1); break;                         // last mantissa bit
        case 2: p[i] = special[rnd() % special.size()]; break;                   // +-0, +-inf, NaNs, denormals
        case 3: p[i] = rnd(); break;                                             // any bits
        case 4: p[i] = bits_of((float)(rnd() % 8) / 8.0f); break;                // many ties
        default: p[i] = bits_of((float)(rnd() & 0xffffff) / 16777216.0f); break;  // gate weights in [0, 1)
      }
    }
    check_segment(p, idx, true);
  }
  // ---- large segments with a constant priority: indices through the third index byte, both strides
  for (uint32_t stride : {1u, 2u}) {
    const size_t n = 70000;
    std::vector<uint32_t> p(n, bits_of(0.125f)), idx(n);
    for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i * stride + (stride - 1);
    check_segment(p, idx, false);
  }
  {
    const size_t n = 50000;
    std::vector<uint32_t> p(n), idx(n);
    for (size_t i = 0; i < n; ++i) {
      idx[i] = (uint32_t)i * 3;
      p[i] = bits_of((float)(rnd() & 0xffff) / 65536.0f);
    }
    check_segment(p, idx, false);
  }
  if (failures) {
    std::printf("FAILED %d checks\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
