// Stand-alone CPU test of the tile map of the grouped expert GEMM (moe_gemm_map.hpp): for every table
// below and every block id of the grids a launcher would build it walks the map and checks invariants
// I1 .. I4 of the header.  Built by tests/test_moe_gemm_map_cpu.py with -fsanitize=address,undefined
// (the tables live in exactly sized heap arrays, so a read past one is an error).  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "moe_gemm_map.hpp"

namespace gm = mp4x::gemm_map;

struct Seg {
  int64_t group, first, count;
};

struct Case {
  const char* name;
  int layout;
  std::vector<int64_t> table;      // ragged: offsets [G + 1]; padded: valid [G * B]
  int64_t R, G, B, S;
  std::vector<Seg> want;           // the clamped segments, written out from the rule (empty ones left out)
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
  Case c{name, gm::kRagged, {0}, 0, (int64_t)lengths.size(), 1, 1, {}};
  for (size_t g = 0; g < lengths.size(); ++g) {
    if (lengths[g]) c.want.push_back({(int64_t)g, c.R, lengths[g]});
    c.R += lengths[g];
    c.table.push_back(c.R);
  }
  c.R += tail;
  return c;
}

static Case padded(const char* name, std::vector<std::vector<int64_t>> valid, int64_t S, std::vector<int64_t> clamped) {
  Case c{name, gm::kPadded, {}, 0, (int64_t)valid.size(), (int64_t)valid[0].size(), S, {}};
  for (auto& row : valid)
    for (int64_t v : row) c.table.push_back(v);
  c.R = c.G * c.B * S;
  for (size_t s = 0; s < clamped.size(); ++s)
    if (clamped[s]) c.want.push_back({(int64_t)s / c.B, (int64_t)s * S, clamped[s]});
  return c;
}

static void run(const Case& c, int64_t BM, int64_t BK) {
  // the table in an exactly sized heap block: the sanitizer sees any read outside it
  int64_t* table = (int64_t*)std::malloc(c.table.size() * sizeof(int64_t));
  for (size_t i = 0; i < c.table.size(); ++i) table[i] = c.table[i];
  std::vector<int> owner(c.R, -1), computed(c.R, 0), zeroed(c.R, 0);
  for (const Seg& s : c.want)
    for (int64_t r = s.first; r < s.first + s.count; ++r) owner[r] = (int)s.group;

  // forward: every block id of the host's grid, and a few past it (those must be empty)
  const int64_t tiles = gm::row_tiles(c.layout, c.R, c.G, c.B, c.S, BM);
  CHECK(tiles >= 0 && tiles <= c.R + c.G * c.B, "row tiles %lld", (long long)tiles);
  for (int64_t tile = 0; tile < tiles + 3; ++tile) {
    const gm::Item it = gm::forward_item(c.layout, table, c.R, c.G, c.B, c.S, BM, tile);
    CHECK(it.trips <= c.G + 1, "trips %lld", (long long)it.trips);                                       // I1
    CHECK(it.compute >= 0 && it.zero >= 0 && it.compute + it.zero <= BM, "tile %lld", (long long)tile);
    if (it.compute + it.zero == 0) continue;
    CHECK(tile < tiles, "tile %lld past the grid has work", (long long)tile);
    CHECK(it.first >= 0 && it.first + it.compute + it.zero <= c.R, "rows of tile %lld", (long long)tile);  // I2
    CHECK(it.group >= 0 && it.group < c.G, "group of tile %lld", (long long)tile);
    if (!(it.first >= 0 && it.first + it.compute + it.zero <= c.R)) continue;
    for (int64_t r = it.first; r < it.first + it.compute; ++r) {
      CHECK(owner[r] == it.group, "row %lld computed for group %lld", (long long)r, (long long)it.group);
      computed[r] += 1;
    }
    for (int64_t r = it.first + it.compute; r < it.first + it.compute + it.zero; ++r) zeroed[r] += 1;
  }
  for (int64_t r = 0; r < c.R; ++r) {                                                                   // I3
    CHECK(computed[r] == (owner[r] >= 0 ? 1 : 0), "row %lld computed %d times", (long long)r, computed[r]);
    CHECK(zeroed[r] == (owner[r] >= 0 ? 0 : 1), "row %lld zeroed %d times", (long long)r, zeroed[r]);
  }

  // weight gradient: every group's walk gives its segments, in row order, inside the step bound
  const int64_t max_steps = gm::wgrad_max_steps(c.layout, c.R, c.B, c.S, BK);
  for (int64_t g = 0; g < c.G; ++g) {
    gm::Walk w = gm::wgrad_walk_init(c.layout, table, c.R, c.G, c.B, g);
    CHECK(w.trips <= c.G, "init trips %lld", (long long)w.trips);
    std::vector<int64_t> rows, want;
    for (const Seg& s : c.want)
      if (s.group == g)
        for (int64_t r = s.first; r < s.first + s.count; ++r) want.push_back(r);
    int64_t steps = 0, row0 = 0, nrows = 0;
    for (int64_t guard = 0; guard <= max_steps; ++guard) {
      if (!gm::wgrad_next(c.layout, table, c.B, c.S, g, BK, w, row0, nrows)) break;
      CHECK(w.trips <= c.B + 1, "next trips %lld", (long long)w.trips);
      CHECK(nrows >= 1 && nrows <= BK && row0 >= 0 && row0 + nrows <= c.R, "step %lld of group %lld",
            (long long)steps, (long long)g);
      if (!(nrows >= 1 && nrows <= BK && row0 >= 0 && row0 + nrows <= c.R)) break;
      for (int64_t r = row0; r < row0 + nrows; ++r) rows.push_back(r);
      ++steps;
    }
    CHECK(steps <= max_steps, "group %lld: %lld steps, bound %lld", (long long)g, (long long)steps,
          (long long)max_steps);
    CHECK(!gm::wgrad_next(c.layout, table, c.B, c.S, g, BK, w, row0, nrows), "group %lld: the walk goes on",
          (long long)g);
    CHECK(rows == want, "group %lld: the walk's rows differ (%zu, want %zu)", (long long)g, rows.size(), want.size());
  }
  std::free(table);
}

int main() {
  const int64_t big = (int64_t)1 << 62;
  std::vector<Case> cases;
  // the layouts of tests/test_moe_gemm_cpu.py
  cases.push_back(ragged("ragged [0,17,5,1,40]+3", {0, 17, 5, 1, 40}, 3));
  cases.push_back(ragged("ragged [9,0]", {9, 0}, 0));
  cases.push_back(ragged("ragged [0,0]+4", {0, 0}, 4));
  cases.push_back(padded("padded 3x3 S=8", {{0, 1, 7}, {8, 9, 300}, {0, 0, 0}}, 8, {0, 1, 7, 8, 8, 8, 0, 0, 0}));
  cases.push_back(padded("padded [[3,11]] S=11", {{3, 11}}, 11, {3, 11}));
  // around one and two row tiles, a long group, a padded share past one tile
  cases.push_back(ragged("ragged [127,128,129,0,300]+2", {127, 128, 129, 0, 300}, 2));
  cases.push_back(ragged("ragged [1100]", {1100}, 0));
  cases.push_back(padded("padded [[130,0],[64,129]] S=130", {{130, 0}, {64, 129}}, 130, {130, 0, 64, 129}));
  // hostile tables: c = [0, 9, 9, 20, 20] over R = 20, and c = [0, 0, 7, 7, 7] over R = 9
  cases.push_back(Case{"ragged offsets [5,9,4,1000,12] R=20", gm::kRagged, {5, 9, 4, 1000, 12}, 20, 4, 1, 1,
                       {{0, 0, 9}, {2, 9, 11}}});
  cases.push_back(Case{"ragged offsets [0,-3,7,7,-1] R=9", gm::kRagged, {0, -3, 7, 7, -1}, 9, 4, 1, 1, {{1, 0, 7}}});
  cases.push_back(padded("padded valid [-5, 2^62, S+1, 3] S=6", {{-5, big}, {7, 3}}, 6, {0, 6, 6, 3}));
  cases.push_back(Case{"ragged offsets [2^62, -2^62, 2^62] R=5", gm::kRagged, {big, -big, big}, 5, 2, 1, 1,
                       {{1, 0, 5}}});
  const int64_t BMs[] = {64, 128, 16}, BKs[] = {64, 32, 5};
  for (const Case& c : cases)
    for (int64_t BM : BMs)
      for (int64_t BK : BKs) run(c, BM, BK);
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("OK %zu tables\n", cases.size());
  return 0;
}
