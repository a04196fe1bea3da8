// Stand-alone CPU test of the row rule of the gated expert activation (moe_act_map.hpp): for every
// table below, every item count and a few grids it walks every wave and lane as a kernel would and
// checks invariants J1 .. J4 of the header.  Built by tests/test_moe_act_map_cpu.py with
// -fsanitize=address,undefined (the tables live in exactly sized heap arrays, so a read past one is
// an error).  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "moe_act_map.hpp"

namespace am = mp4x::act_map;

struct Case {
  const char* name;
  int layout;
  std::vector<int64_t> table;      // ragged: offsets [G + 1]; padded: valid [G * B]
  int64_t R, G, B, S;
};

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s: ", c.name);                   \
      std::printf(__VA_ARGS__);                           \
      std::printf(" (%s, line %d)\n", #cond, __LINE__);   \
      if (++failures > 20) std::exit(1);                  \
    }                                                     \
  } while (0)

static Case ragged(const char* name, std::vector<int64_t> lengths, int64_t tail) {
  Case c{name, am::kRagged, {0}, 0, (int64_t)lengths.size(), 1, 1};
  for (int64_t n : lengths) {
    c.R += n;
    c.table.push_back(c.R);
  }
  c.R += tail;
  return c;
}

static Case padded(const char* name, std::vector<std::vector<int64_t>> valid, int64_t S) {
  Case c{name, am::kPadded, {}, 0, (int64_t)valid.size(), (int64_t)valid[0].size(), S};
  for (auto& row : valid)
    for (int64_t v : row) c.table.push_back(v);
  c.R = c.G * c.B * S;
  return c;
}

// The rule as mp4x.parallel.moe._table_segments writes it: the sequential recurrence, segment by segment.
static std::vector<int> owned_by_rule(const Case& c) {
  std::vector<int> own(c.R, 0);
  if (c.layout == am::kRagged) {
    int64_t prev = 0;
    for (int64_t g = 0; g < c.G; ++g) {
      int64_t hi = c.table[g + 1] < c.R ? c.table[g + 1] : c.R;
      if (hi < prev) hi = prev;
      for (int64_t r = prev; r < hi; ++r) own[r] = 1;
      prev = hi;
    }
    return own;
  }
  for (int64_t s = 0; s < c.G * c.B; ++s) {
    int64_t n = c.table[s] < c.S ? c.table[s] : c.S;
    if (n < 0) n = 0;
    for (int64_t r = s * c.S; r < s * c.S + n; ++r) own[r] = 1;
  }
  return own;
}

static void run(const Case& c, int64_t nitems, int64_t nwaves) {
  // the table in an exactly sized heap block: the sanitizer sees any read outside it
  int64_t* table = (int64_t*)std::malloc((c.table.size() ? c.table.size() : 1) * sizeof(int64_t));
  for (size_t i = 0; i < c.table.size(); ++i) table[i] = c.table[i];
  const std::vector<int> want = owned_by_rule(c);
  const am::Shape s = am::shape(nitems);
  CHECK(s.lanes >= 1 && s.lanes <= am::kWave && (1 << s.lg) == s.lanes && s.rows * s.lanes == am::kWave, "shape of %lld",
        (long long)nitems);
  CHECK(s.lanes == am::kWave || (int64_t)s.lanes * am::kItems >= nitems, "lanes %d for %lld items", s.lanes, (long long)nitems);
  CHECK(c.R < am::kMaxRows && c.G <= am::kMaxGroups, "limits");

  // the fold of c[G]: every lane's part, joined in two different orders
  int64_t end = 0, end_rev = 0;
  if (c.layout == am::kRagged) {
    int64_t parts[am::kWave];
    for (int lane = 0; lane < am::kWave; ++lane) {
      int64_t trips = 0;
      parts[lane] = am::ragged_end_part(table, c.G, c.R, lane, trips);
      CHECK(trips <= (c.G + am::kWave - 1) / am::kWave && trips <= am::kMaxGroups / am::kWave, "fold trips %lld",
            (long long)trips);                                                                       // J1
      CHECK(parts[lane] >= 0 && parts[lane] <= c.R, "part %lld", (long long)parts[lane]);
    }
    for (int lane = 0; lane < am::kWave; ++lane) end = am::ragged_end_join(end, parts[lane]);
    for (int lane = am::kWave - 1; lane >= 0; --lane) end_rev = am::ragged_end_join(parts[lane], end_rev);
    CHECK(end == end_rev && end >= 0 && end <= c.R, "c[G] = %lld / %lld", (long long)end, (long long)end_rev);
  }

  std::vector<int> seen((size_t)(c.R * nitems), 0);
  const int64_t max_blocks = (am::row_blocks(c.R, s.rows) + nwaves - 1) / nwaves;
  const int64_t max_items = (nitems + s.lanes - 1) / s.lanes;
  for (int64_t wave = 0; wave < nwaves; ++wave) {
    int64_t blocks = 0;
    for (int64_t r0 = wave * s.rows; r0 < c.R; r0 += nwaves * s.rows) {
      ++blocks;
      for (int lane = 0; lane < am::kWave; ++lane) {
        int sub = -1;
        const int64_t r = am::lane_row(s, r0, c.R, lane, sub);
        CHECK(sub >= 0 && sub < s.lanes, "sub %d", sub);
        if (r < 0) continue;
        CHECK(r >= r0 && r < c.R && r < r0 + s.rows, "row %lld of block %lld", (long long)r, (long long)r0);   // J2
        if (!(r >= 0 && r < c.R)) continue;
        bool own;
        if (c.layout == am::kRagged) {
          own = r < end;
        } else {
          uint32_t seg = ~0u;
          own = am::padded_owned(table, (uint32_t)r, (uint32_t)c.S, seg);
          CHECK((int64_t)seg < c.G * c.B && (int64_t)seg == r / c.S, "segment %u of row %lld", seg, (long long)r);
        }
        CHECK((int)own == want[r], "row %lld owned %d, the rule says %d", (long long)r, (int)own, want[r]);   // J3
        int64_t items = 0;
        for (int64_t v0 = sub; v0 < nitems; v0 += (int64_t)s.lanes * am::kItems) {
          for (int i = 0; i < am::kItems; ++i) {
            const int64_t v = v0 + (int64_t)i * s.lanes;
            if (v >= nitems) continue;
            ++items;
            seen[(size_t)(r * nitems + v)] += 1;
          }
        }
        CHECK(items <= max_items, "row %lld: %lld items in a lane, bound %lld", (long long)r, (long long)items,
              (long long)max_items);                                                                 // J1
      }
    }
    CHECK(blocks <= max_blocks, "wave %lld: %lld row blocks, bound %lld", (long long)wave, (long long)blocks,
          (long long)max_blocks);                                                                    // J1
  }
  for (size_t i = 0; i < seen.size(); ++i)
    CHECK(seen[i] == 1, "row %lld item %lld visited %d times", (long long)(i / nitems), (long long)(i % nitems), seen[i]);
  std::free(table);
}

int main() {
  const int64_t big = (int64_t)1 << 62;
  std::vector<Case> cases;
  // the tables of tests/moe_glu_ref.py
  cases.push_back(padded("padded [[0,5],[7,-1],[3,1]] S=5", {{0, 5}, {7, -1}, {3, 1}}, 5));
  cases.push_back(padded("padded [[1]] S=1", {{1}}, 1));
  cases.push_back(padded("padded [[0]] S=1", {{0}}, 1));
  {
    // valid in [-2, 75] from a fixed recurrence: below 0, inside [0, S] and above S all occur
    std::vector<std::vector<int64_t>> valid(2, std::vector<int64_t>(4));
    uint64_t x = 12345;
    for (auto& row : valid)
      for (int64_t& v : row) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v = (int64_t)((x >> 33) % 78) - 2;
      }
    valid[0][0] = -2;
    valid[1][3] = 75;
    cases.push_back(padded("padded 2x4 S=70", valid, 70));
  }
  cases.push_back(ragged("ragged [0,3,65,0,1]", {0, 3, 65, 0, 1}, 0));
  cases.push_back(ragged("ragged [0,3,65,0,1]+4", {0, 3, 65, 0, 1}, 4));
  cases.push_back(Case{"ragged offsets [5,9,4,1000,12] R=20", am::kRagged, {5, 9, 4, 1000, 12}, 20, 4, 1, 1});
  cases.push_back(Case{"ragged offsets [0,-3,7,7,-1] R=9", am::kRagged, {0, -3, 7, 7, -1}, 9, 4, 1, 1});
  cases.push_back(ragged("ragged R=0", {0, 0}, 0));
  cases.push_back(Case{"ragged G=0 R=3", am::kRagged, {0}, 3, 0, 1, 1});
  // hostile entries, and more groups than one trip of the fold
  cases.push_back(padded("padded valid [-2^62, 2^62, S+1, 3] S=6", {{-big, big}, {7, 3}}, 6));
  cases.push_back(Case{"ragged offsets [2^62, -2^62, 3, -1] R=5", am::kRagged, {big, -big, 3, -1}, 5, 3, 1, 1});
  {
    std::vector<int64_t> lengths(200, 0);
    lengths[3] = 2;
    lengths[130] = 5;
    lengths[199] = 1;
    cases.push_back(ragged("ragged 200 groups +2", lengths, 2));
  }
  // items a row: N in {1, 7, 8, 24, 260, 1024} as elements, as 4-element and as 8-element vectors
  const int64_t items[] = {1, 2, 3, 6, 7, 8, 24, 65, 128, 256, 260, 1024};
  const int64_t grids[] = {4, 12, 8192};
  for (const Case& c : cases)
    for (int64_t n : items)
      for (int64_t w : grids) run(c, n, w);
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("OK %zu tables\n", cases.size());
  return 0;
}
