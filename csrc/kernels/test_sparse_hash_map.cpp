// Stand-alone CPU test of csrc/kernels/sparse_hash_map.hpp (build with -fsanitize=address,undefined):
// the priority insertion of K5c, run as k_hashc_insert runs it (a lane = a carried key, a slot, the
// value read there; one memory access per step: the read, or the CAS that hmap::step asks for),
// from many shuffled row orders one lane at a time, and with several lanes taking single steps in
// turn (round robin and at random), against the definition: plain linear probing of the distinct
// keys in ascending unsigned order.  t = 1024 slots with 1 to 512 rows, duplicate keys, keys with
// the top bit set, a set whose homes all lie in the last 8 slots (the probes wrap round) and a set
// with one common home (one long cluster).  The advance bound is never reached, the step bound
// never passed, and the read-only probe of k_hashc_link finds every key before an empty slot.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "sparse_hash_map.hpp"

using namespace mp4x;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (++failures < 20) std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                   \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static void shuffle(std::vector<uint64_t>& a) {
  for (size_t i = a.size(); i > 1; --i) std::swap(a[i - 1], a[rnd() % i]);
}

// The definition.
static std::vector<uint64_t> canonical(std::vector<uint64_t> rows, int64_t t) {
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  std::vector<uint64_t> T((size_t)t, hmap::kEmpty);
  for (uint64_t k : rows) {
    uint64_t h = hmap::home(k, (uint64_t)t - 1);
    while (T[h] != hmap::kEmpty) h = (h + 1) & ((uint64_t)t - 1);
    T[h] = k;
  }
  return T;
}

struct Lane {
  uint64_t v = 0, h = 0, c = 0, adv = 0, it = 0;
  bool have_c = false, live = false, gave_up = false;
};

static uint64_t max_adv = 0, max_it = 0;

static void start(Lane& l, uint64_t key, uint64_t mask) {
  l = Lane();
  l.v = key;
  l.h = hmap::home(key, mask);
  l.live = true;
}

// One memory access of the lane (k_hashc_insert's loop, cut at every access to the table).
static void one_step(Lane& l, std::vector<uint64_t>& T, uint64_t mask, uint64_t amax, uint64_t imax) {
  if (!l.have_c) {                                       // the relaxed load
    l.c = T[l.h];
    l.have_c = true;
    return;
  }
  if (++l.it > imax) {
    l.gave_up = true;
    l.live = false;
    return;
  }
  max_it = std::max(max_it, l.it);
  const int act = hmap::step(l.c, l.v);
  if (act == hmap::kDone) {
    l.live = false;
    return;
  }
  if (act == hmap::kSwap) {                            // the CAS: this step's one access
    const uint64_t old = T[l.h];
    if (old != l.c) {
      l.c = old;                                       // lost: step again on the new value,
      return;                                          // which may CAS again: the next step
    }
    T[l.h] = l.v;
    if (l.c == hmap::kEmpty) {
      l.live = false;
      return;
    }
    l.v = l.c;
  }
  if (++l.adv >= amax) {
    l.gave_up = true;
    l.live = false;
    return;
  }
  max_adv = std::max(max_adv, l.adv);
  l.h = (l.h + 1) & mask;
  l.have_c = act == hmap::kAdvance;                    // after a CAS the load there is the next step
  if (l.have_c) l.c = T[l.h];
  return;
}

// rows inserted by `lanes` lanes; pick = 0: each lane to completion, 1: round robin, 2: random lane.
static std::vector<uint64_t> insert(const std::vector<uint64_t>& rows, int64_t t, int lanes, int pick) {
  const uint64_t mask = (uint64_t)t - 1;
  const uint64_t amax = hmap::advance_bound(t), imax = hmap::iter_bound((int64_t)rows.size(), t);
  std::vector<uint64_t> T((size_t)t, hmap::kEmpty);
  std::vector<Lane> L((size_t)lanes);
  size_t nextrow = 0, live = 0, turn = 0;
  for (;;) {
    for (auto& l : L)
      if (!l.live && nextrow < rows.size()) {
        start(l, rows[nextrow++], mask);
        ++live;
      }
    if (!live) break;
    size_t j = pick == 2 ? rnd() % L.size() : turn++ % L.size();
    while (!L[j].live) j = (j + 1) % L.size();
    do {
      one_step(L[j], T, mask, amax, imax);
      CHECK(!L[j].gave_up);
    } while (pick == 0 && L[j].live);
    if (!L[j].live) --live;
  }
  return T;
}

static void check_link(const std::vector<uint64_t>& rows, const std::vector<uint64_t>& T, int64_t t) {
  const uint64_t mask = (uint64_t)t - 1;
  for (uint64_t k : rows) {
    uint64_t h = hmap::home(k, mask), adv = 0;
    uint64_t cur = T[h];
    while (cur != k && cur != hmap::kEmpty && ++adv < hmap::advance_bound(t)) {
      h = (h + 1) & mask;
      cur = T[h];
    }
    CHECK(cur == k);
  }
}

static void run_case(const std::vector<uint64_t>& rows_in, int shuffles) {
  const int64_t t = hmap::table_slots((int64_t)rows_in.size());
  CHECK(t == 1024);
  const std::vector<uint64_t> want = canonical(rows_in, t);
  size_t filled = 0;
  for (uint64_t x : want) filled += x != hmap::kEmpty;
  CHECK(filled <= (size_t)t / 2);
  check_link(rows_in, want, t);
  std::vector<uint64_t> rows = rows_in;
  for (int s = 0; s < shuffles; ++s) {
    shuffle(rows);
    CHECK(insert(rows, t, 1, 0) == want);
    const int lanes[] = {2, 7, 64, 256};
    CHECK(insert(rows, t, lanes[s % 4], 1) == want);
    CHECK(insert(rows, t, lanes[(s + 1) % 4], 2) == want);
  }
  std::sort(rows.begin(), rows.end());                   // ascending and descending row orders too
  CHECK(insert(rows, t, 1, 0) == want);
  CHECK(insert(rows, t, 64, 1) == want);
  std::reverse(rows.begin(), rows.end());
  CHECK(insert(rows, t, 1, 0) == want);
  CHECK(insert(rows, t, 64, 1) == want);
}

int main() {
  CHECK(hmap::table_slots(0) == 1024 && hmap::table_slots(512) == 1024 && hmap::table_slots(513) == 2048);
  CHECK(hmap::table_slots((1ll << 30) - 1) == (1ll << 31));
  CHECK(hmap::step(5, 5) == hmap::kDone && hmap::step(4, 5) == hmap::kAdvance && hmap::step(6, 5) == hmap::kSwap);
  CHECK(hmap::step(hmap::kEmpty, 0x8000000000000000ull) == hmap::kSwap);       // EMPTY loses to every key
  CHECK(hmap::step(1, 0x8000000000000000ull) == hmap::kAdvance);               // unsigned order
  CHECK(hmap::iter_bound((1ll << 30) - 1, 1ll << 31) > (1ull << 58));          // no overflow at the largest n

  const uint64_t top = 0x8000000000000000ull;
  const int sizes[] = {1, 2, 3, 7, 64, 300, 512};
  for (int n : sizes) {
    std::vector<uint64_t> distinct, dup, neg;
    for (int i = 0; i < n; ++i) distinct.push_back(rnd() >> 1);
    for (int i = 0; i < n; ++i) dup.push_back(distinct[rnd() % (size_t)((n + 2) / 3)]);      // every key ~3 times
    for (int i = 0; i < n; ++i) neg.push_back((i & 1) ? (rnd() | top) : (uint64_t)(-2 - (int64_t)(rnd() % 50)));
    run_case(distinct, n <= 64 ? 40 : 12);
    run_case(dup, n <= 64 ? 40 : 12);
    run_case(neg, n <= 64 ? 40 : 12);
  }
  {                                                      // homes in the last 8 slots: the probes wrap
    std::vector<uint64_t> wrap;
    for (uint64_t k = 1; wrap.size() < 300; ++k)
      if (hmap::home(k * 0x10001ull, 1023) >= 1016) wrap.push_back(k * 0x10001ull);
    run_case(wrap, 12);
    for (int i = 0; i < 200; ++i) wrap.push_back(wrap[rnd() % 300]);
    run_case(wrap, 12);
    const std::vector<uint64_t> T = canonical(wrap, 1024);
    CHECK(T[0] != hmap::kEmpty && T[1015] == hmap::kEmpty);                    // it did wrap
  }
  {                                                      // one common home: one cluster of 400
    std::vector<uint64_t> one;
    for (uint64_t k = 1; one.size() < 400; ++k)
      if (hmap::home(k | top, 1023) == 700) one.push_back(k | top);
    run_case(one, 8);
  }
  CHECK(max_adv < 1024 / 2 + 1);                         // far from the advance bound t
  if (failures) {
    std::printf("FAILED %d checks\n", failures);
    return 1;
  }
  std::printf("OK max advances %llu, max steps %llu\n", (unsigned long long)max_adv, (unsigned long long)max_it);
  return 0;
}
