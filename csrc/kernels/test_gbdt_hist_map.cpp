// Stand-alone CPU test of the tile map of the GBDT histogram (gbdt_hist_map.hpp): for every table
// below and a few (F, B) it builds c and T as the kernel does and walks every block id and every
// thread of the grid a launch would build, and checks invariants H1 .. H3 of the header.  Built by
// tests/test_kernel_maps_cpu.py with -fsanitize=address,undefined (the tables live in exactly
// sized heap arrays, so a read past one is an error).  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gbdt_hist_map.hpp"
#define MAP_TEST_SUBJECT c.name
#include "test_map_common.hpp"

namespace gm = mp4x::gbdt_map;

struct Case {
  const char* name;
  std::vector<int64_t> seg;      // k + 1 entries
  int64_t m;
};

static Case lengths(const char* name, std::vector<int64_t> len, int64_t tail) {
  Case c{name, {0}, 0};
  for (int64_t n : len) {
    c.m += n;
    c.seg.push_back(c.m);
  }
  c.m += tail;
  return c;
}

static void run(const Case& c, int64_t F, int B) {
  const int64_t k = (int64_t)c.seg.size() - 1;
  int64_t* seg = (int64_t*)std::malloc(c.seg.size() * sizeof(int64_t));
  for (size_t i = 0; i < c.seg.size(); ++i) seg[i] = c.seg[i];
  int32_t* cc = (int32_t*)std::malloc((k + 1) * sizeof(int32_t));
  int32_t* T = (int32_t*)std::malloc((k + 1) * sizeof(int32_t));
  CHECK(k <= gm::kMaxNodes && c.m < gm::kMaxRows, "limits");
  gm::build_tables(seg, k, c.m, cc, T);

  // the rule as _table_segments writes it: owner[slot] = node, -1 for a slot nobody owns
  std::vector<int> owner(c.m, -1);
  int64_t prev = 0;
  for (int64_t j = 0; j < k; ++j) {
    int64_t hi = c.seg[j + 1] < c.m ? c.seg[j + 1] : c.m;
    if (hi < prev) hi = prev;
    for (int64_t i = prev; i < hi; ++i) owner[i] = (int)j;
    CHECK(cc[j] == prev && cc[j + 1] == hi, "c[%lld]", (long long)j);                                 // H2
    CHECK(T[j + 1] >= T[j] && T[j + 1] - T[j] == gm::tiles_of(hi - prev), "T[%lld]", (long long)j);
    prev = hi;
  }
  CHECK(T[k] <= gm::max_tiles(c.m, k), "T[k] = %d above the grid's %lld", T[k], (long long)gm::max_tiles(c.m, k));

  const gm::Shape s = gm::shape(F, B);
  CHECK(s.fg >= 1 && s.fg <= gm::kWave && (1 << s.lg) == s.fg && s.rows * s.fg == gm::kWave, "shape");
  CHECK((int64_t)s.fg * B * 16 <= gm::kLdsBytes || s.fg == 1, "LDS of fg = %d", s.fg);
  CHECK(s.fg == 1 || s.fg / 2 < F, "fg = %d for F = %lld", s.fg, (long long)F);
  const int64_t ngroups = gm::groups(F, s.fg), grid = gm::max_tiles(c.m, k) * ngroups;
  const int step = gm::rows_per_step(s);
  const int64_t max_slots = (gm::kTile + step - 1) / step;
  std::vector<int> seen((size_t)(c.m * F), 0);
  for (int64_t block = 0; block < grid; ++block) {
    const gm::Tile t = gm::tile_of(cc, T, (int)k, block, ngroups, F, s);
    if (!t.owns) continue;
    CHECK(t.node >= 0 && t.node < k && t.lo >= cc[t.node] && t.hi <= cc[t.node + 1] && t.hi - t.lo <= gm::kTile,
          "block %lld: node %d slots [%d, %d)", (long long)block, t.node, t.lo, t.hi);                // H2
    CHECK(t.f0 >= 0 && t.f0 < t.f1 && t.f1 <= F && t.f1 - t.f0 <= s.fg, "block %lld: features [%d, %d)",
          (long long)block, t.f0, t.f1);
    int trips = 0;
    gm::find_node(T, (int)k, (int32_t)(block / ngroups), trips);
    CHECK(trips <= 13, "find_node took %d trips", trips);                                             // H1
    if (!(t.node >= 0 && t.node < k && t.lo >= 0 && t.hi <= c.m && t.f0 >= 0 && t.f1 <= F)) continue;
    for (int tid = 0; tid < gm::kWaves * gm::kWave; ++tid) {
      const int f = gm::lane_feature(s, t, tid);
      if (f < 0) continue;
      CHECK(f >= t.f0 && f < t.f1, "feature %d", f);
      if (!(f >= t.f0 && f < t.f1)) continue;
      int64_t slots = 0;
      for (int64_t i = (int64_t)t.lo + gm::lane_row(s, tid); i < t.hi; i += step) {
        ++slots;
        CHECK(owner[i] == t.node, "slot %lld of node %d visited for node %d", (long long)i, owner[i], t.node);   // H3
        seen[(size_t)(i * F + f)] += 1;
      }
      CHECK(slots <= max_slots, "%lld slots in a lane, bound %lld", (long long)slots, (long long)max_slots);      // H1
    }
  }
  for (int64_t i = 0; i < c.m; ++i)
    for (int64_t f = 0; f < F; ++f)
      CHECK(seen[(size_t)(i * F + f)] == (owner[i] >= 0 ? 1 : 0), "slot %lld feature %lld visited %d times",
            (long long)i, (long long)f, seen[(size_t)(i * F + f)]);                                   // H3
  std::free(T);
  std::free(cc);
  std::free(seg);
}

int main() {
  const int64_t big = (int64_t)1 << 62;
  std::vector<Case> cases;
  cases.push_back(lengths("one node 5000", {5000}, 0));
  cases.push_back(lengths("lengths [0,3,4097,0,1]+4", {0, 3, 4097, 0, 1}, 4));
  cases.push_back(lengths("lengths [4096,4096,1]", {4096, 4096, 1}, 0));
  cases.push_back(Case{"seg [5,9,4,1000,12] m=20", {5, 9, 4, 1000, 12}, 20});
  cases.push_back(Case{"seg [0,-3,7,7,-1] m=9", {0, -3, 7, 7, -1}, 9});
  cases.push_back(Case{"seg [2^62,-2^62,3,2^62,-1] m=9000", {big, -big, 3, big, -1}, 9000});
  cases.push_back(lengths("m = 0", {0, 0}, 0));
  cases.push_back(Case{"k = 0, m = 3", {0}, 3});
  {
    std::vector<int64_t> len(64, 0);     // most nodes empty
    len[3] = 2;
    len[40] = 4100;
    len[63] = 1;
    cases.push_back(lengths("64 nodes, 3 live, +2", len, 2));
  }
  {
    std::vector<int64_t> len(gm::kMaxNodes, 1);
    len[100] = 5000;
    cases.push_back(lengths("kMaxNodes nodes", len, 0));
  }
  const int64_t Fs[] = {1, 5, 16, 37};
  const int Bs[] = {2, 16, 255, 256};
  for (const Case& c : cases)
    for (int64_t F : Fs)
      for (int B : Bs) run(c, F, B);
  return map_test::report("OK %zu tables\n", cases.size());
}
