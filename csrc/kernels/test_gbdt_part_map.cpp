// Stand-alone CPU test of the destination map of the GBDT row partition (gbdt_part_map.hpp): for
// every table below it runs the count, offsets and scatter steps of gbdt_level.hip as plain loops over
// every tile, wave, step and lane, through the header's functions and the header's scratch layout,
// and checks invariants P1 .. P3 of the header.  Built by tests/test_kernel_maps_cpu.py with
// -fsanitize=address,undefined (the scratch and the outputs are exactly sized heap arrays, so an
// access past one is an error).  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gbdt_part_map.hpp"
#define MAP_TEST_SUBJECT c.name
#include "test_map_common.hpp"

namespace gm = mp4x::gbdt_map;
namespace gp = mp4x::gbdt_part;

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

// The byte a slot's row would gather (-1: a row index out of range) and the split of a node.
static int bin_of(int64_t slot) { return slot % 11 == 3 ? -1 : (int)((slot * 2654435761u >> 7) & 255); }
static gp::Rule rule_of(int64_t j, int64_t F) {
  const int32_t feats[] = {0, (int32_t)F - 1, -1, 0, (int32_t)F, 0};
  const int32_t thrs[] = {100, -1, 50, 255, 7, 180};
  return gp::rule(feats[j % 6], thrs[j % 6], (int32_t)(j % 3 == 1 ? 5 : 0), F);
}

static void run(const Case& c, int64_t F) {
  const int64_t k = (int64_t)c.seg.size() - 1, m = c.m;
  CHECK(k <= gp::kMaxParents && m < gm::kMaxRows, "limits");
  const gp::Layout l = gp::layout(m, k);
  CHECK(l.tiles == gm::max_tiles(m, k) && l.tab % 16 == 0 && l.scan % 4 == 0 && l.scan >= l.tab + 8 * (uint64_t)(k + 1) &&
            l.bytes == l.scan + 8 * (uint64_t)(l.tiles + 1), "layout");
  char* scratch = (char*)std::malloc(l.bytes);
  int64_t* seg = (int64_t*)std::malloc((k + 1) * sizeof(int64_t));
  for (int64_t j = 0; j <= k; ++j) seg[j] = c.seg[j];
  uint64_t* masks = (uint64_t*)scratch;                  // pairs: [tile][step][2]
  int32_t* cc = (int32_t*)(scratch + l.tab);
  int32_t* T = cc + k + 1;
  int32_t* S = (int32_t*)(scratch + l.scan);
  int32_t* G = S + l.tiles + 1;
  gm::build_tables(seg, k, m, cc, T);
  const gm::Shape one = {1, 0, gm::kWave};

  // count: a block per tile
  for (int64_t b = 0; b < l.tiles; ++b) {
    const gm::Tile t = gm::tile_of(cc, T, (int)k, b, 1, F, one);
    const gp::Rule r = t.owns ? rule_of(t.node, F) : gp::rule(-1, 0, 0, F);
    CHECK(!r.splits || (r.f >= 0 && r.f < F), "feature %lld of node %d", (long long)r.f, t.node);
    int nf = 0, ns = 0;
    for (int w = 0; w < gm::kWaves; ++w)
      for (int s = gp::first_step(w); s < gp::first_step(w) + gp::kWaveSteps; ++s) {
        uint64_t fm = 0, sm = 0;
        for (int lane = 0; lane < gm::kWave; ++lane) {
          const int64_t i = gp::slot_of(t, s, lane);
          const int sd = t.owns ? gp::side(r, i < t.hi ? bin_of(i) : -1) : 0;
          if (sd == 1) fm |= (uint64_t)1 << lane;
          if (sd == 2) sm |= (uint64_t)1 << lane;
        }
        nf += gp::bits(fm);
        ns += gp::bits(sm);
        if (t.owns) {
          masks[(b * gp::kSteps + s) * 2] = fm;
          masks[(b * gp::kSteps + s) * 2 + 1] = sm;
        }
      }
    S[b] = nf;
    G[b] = ns;
  }

  // offsets: scan_passes passes of kScan tiles
  int32_t run_s = 0, run_g = 0;
  const int64_t passes = gp::scan_passes(l.tiles);
  CHECK(passes * gp::kScan >= l.tiles && passes <= gm::max_tiles(m, k) / gp::kScan + 1, "passes");      // P1
  for (int64_t p = 0; p < passes; ++p)
    for (int tid = 0; tid < gp::kScan; ++tid) {
      const int64_t t = p * gp::kScan + tid;
      if (t >= l.tiles) continue;
      const int32_t a = S[t], b = G[t];
      S[t] = run_s;
      G[t] = run_g;
      run_s += a;
      run_g += b;
    }
  S[l.tiles] = run_s;
  G[l.tiles] = run_g;
  int64_t* seg2 = (int64_t*)std::malloc((2 * k + 1) * sizeof(int64_t));
  for (int64_t j = 0; j <= k; ++j) {
    const int64_t tj = gp::scan_index(T[j], l.tiles);
    if (j < k) seg2[j] = S[tj];
    seg2[k + j] = (int64_t)run_s + G[tj];
  }
  const int64_t total = seg2[2 * k];
  CHECK(seg2[0] == 0 && total <= m && total == (int64_t)run_s + run_g, "seg2 ends at %lld", (long long)total);   // P2
  for (int64_t j = 0; j < 2 * k; ++j) CHECK(seg2[j] <= seg2[j + 1], "seg2[%lld]", (long long)j);

  // scatter: a block per tile; out[d] = the slot that went there
  int64_t* out = (int64_t*)std::malloc((total ? total : 1) * sizeof(int64_t));
  std::vector<int> writers((size_t)total, 0);
  for (int64_t b = 0; b < l.tiles; ++b) {
    const gm::Tile t = gm::tile_of(cc, T, (int)k, b, 1, F, one);
    if (!t.owns) continue;
    int ef[gp::kSteps], es[gp::kSteps], nf = 0, ns = 0;
    for (int s = 0; s < gp::kSteps; ++s) {
      ef[s] = nf;
      es[s] = ns;
      nf += gp::bits(masks[(b * gp::kSteps + s) * 2]);
      ns += gp::bits(masks[(b * gp::kSteps + s) * 2 + 1]);
    }
    const int64_t base_f = S[b], base_s = (int64_t)S[l.tiles] + G[b];
    for (int s = 0; s < gp::kSteps; ++s)
      for (int lane = 0; lane < gm::kWave; ++lane) {
        const uint64_t fm = masks[(b * gp::kSteps + s) * 2], sm = masks[(b * gp::kSteps + s) * 2 + 1];
        const bool first = (fm >> lane) & 1, second = (sm >> lane) & 1;
        if (!first && !second) continue;
        CHECK(!(first && second), "tile %lld step %d lane %d on both sides", (long long)b, s, lane);
        const int64_t d = first ? gp::dest(base_f, ef[s], fm, lane) : gp::dest(base_s, es[s], sm, lane);
        CHECK(gp::writable(d, m) && d < total, "destination %lld of %lld", (long long)d, (long long)total);   // P3
        if (d < 0 || d >= total) continue;
        writers[(size_t)d] += 1;
        out[d] = gp::slot_of(t, s, lane);
      }
  }
  for (int64_t d = 0; d < total; ++d) CHECK(writers[(size_t)d] == 1, "slot %lld has %d writers", (long long)d, writers[d]);

  // the definition: per node the first and the second slots in slot order
  int64_t prev = 0;
  std::vector<std::vector<int64_t>> want((size_t)(2 * k));
  for (int64_t j = 0; j < k; ++j) {
    int64_t hi = c.seg[j + 1] < m ? c.seg[j + 1] : m;
    if (hi < prev) hi = prev;
    const gp::Rule r = rule_of(j, F);
    for (int64_t i = prev; i < hi; ++i) {
      const int b = bin_of(i);
      if (!r.splits || b < 0) continue;
      want[(size_t)(((b > r.thr) == r.first_right) ? j : k + j)].push_back(i);
    }
    prev = hi;
  }
  for (int64_t j = 0; j < 2 * k; ++j) {
    const std::vector<int64_t>& w = want[(size_t)j];
    CHECK(seg2[j + 1] - seg2[j] == (int64_t)w.size(), "segment %lld holds %lld, wants %zu", (long long)j,
          (long long)(seg2[j + 1] - seg2[j]), w.size());                                                // P2
    if (seg2[j + 1] - seg2[j] != (int64_t)w.size() || seg2[j] < 0 || seg2[j + 1] > total) continue;
    CHECK(w.empty() || std::memcmp(out + seg2[j], w.data(), w.size() * sizeof(int64_t)) == 0, "order of segment %lld",
          (long long)j);
  }
  std::free(out);
  std::free(seg2);
  std::free(seg);
  std::free(scratch);
}

int main() {
  const int64_t big = (int64_t)1 << 62;
  std::vector<Case> cases;
  cases.push_back(lengths("one node 5000", {5000}, 0));
  cases.push_back(lengths("lengths [0,3,4097,0,1,70]+4", {0, 3, 4097, 0, 1, 70}, 4));
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
    len[61] = 1;
    cases.push_back(lengths("64 nodes, 3 live, +2", len, 2));
  }
  {
    std::vector<int64_t> len(gp::kMaxParents, 1);
    len[100] = 5000;
    cases.push_back(lengths("kMaxParents nodes", len, 0));
  }
  cases.push_back(lengths("two scan passes", {400000, (int64_t)(gp::kScan + 1) * gm::kTile + 17 - 400000}, 0));
  const int64_t Fs[] = {1, 37};
  for (const Case& c : cases)
    for (int64_t F : Fs) run(c, F);
  return map_test::report("OK %zu tables\n", cases.size());
}
