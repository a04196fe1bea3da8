// Destination map of the GBDT row partition (K17, gbdt_level.hip): which wave step of which tile
// holds which row slot, which side a slot falls on, and where the scatter writes it.  Plain C++ (no
// HIP types), the same code on the host and on the device: csrc/kernels/test_gbdt_part_map.cpp walks
// it on the CPU.  The segment table and the tiles are gbdt_hist_map.hpp's, unchanged, with one
// feature group: a tile is kTile = 4096 row slots of one node.
//
// A tile is kSteps = 64 wave steps of 64 slots; wave w of the block takes the kWaveSteps = 16
// consecutive steps from first_step(w), so the slots of a wave are one contiguous run of the tile and
// its first (and its second) rows leave as one contiguous run of the output.  Step s of tile t keeps
// one pair of 64-bit masks (first, second) at masks[t * kSteps + s]: bit l is slot lo + 64 s + l.  A
// slot past the tile's end, a row index outside [0, n) and every slot of a node that does not split
// set neither bit.
//
// Output: seg2 int64[2k + 1].  With S[t], G[t] the exclusive scans of the per-tile first and second
// counts in tile order (tile order is node-major) and Stot, Gtot their totals,
//   seg2[j] = S[T[j]],  seg2[k + j] = Stot + G[T[j]]  (j <= k),
// the first rows of tile t start at S[t], its second rows at Stot + G[t]; inside a tile a slot's
// destination is the tile's base + the bits of the earlier steps + the bits of the lower lanes of its
// own step (dest): slot order, so the partition is stable without an atomic.
//
// Invariants (asserted by the stand-alone test for every table it holds):
//   P1  every loop has a host-known trip count: kWaveSteps steps a wave, scan_passes(tiles) passes of
//       the offsets scan;
//   P2  seg2 is non-decreasing from 0, seg2[2k] <= m, and segment j (k + j) holds exactly the first
//       (second) rows of node j in slot order;
//   P3  every output slot in [0, seg2[2k]) has exactly one writer and nothing is written outside it.
#pragma once
#include "gbdt_hist_map.hpp"

namespace mp4x {
namespace gbdt_part {

namespace gm = gbdt_map;

constexpr int kMaxParents = gm::kMaxNodes / 2;       // k: the 2k children stay a histogram table
constexpr int kSteps = gm::kTile / gm::kWave;        // wave steps (mask pairs) a tile
constexpr int kWaveSteps = kSteps / gm::kWaves;      // consecutive steps a wave
constexpr int kScan = 256;                           // tiles a pass of the offsets scan (one a thread)
static_assert(kSteps == gm::kWave, "one lane of a wave holds one step's masks of a whole tile");

// The scratch of a call: mask pairs | c, T (int32[k + 1] each) | S, G (int32[tiles + 1] each).
struct Layout {
  int64_t tiles;                    // max_tiles(m, k): the grid and the scan length
  uint64_t tab, scan, bytes;        // byte offsets (the masks stand at 0) and the total
};
MP4X_GBDT_HD Layout layout(int64_t m, int64_t k) {
  Layout l;
  l.tiles = gm::max_tiles(m, k);
  l.tab = (uint64_t)l.tiles * kSteps * 16;
  l.scan = l.tab + (uint64_t)(2 * (k + 1)) * 4;
  l.bytes = l.scan + (uint64_t)(2 * (l.tiles + 1)) * 4;
  return l;
}
MP4X_GBDT_HD int64_t scan_passes(int64_t tiles) { return tiles / kScan + 1; }

// The split of a node, read once and clamped: a feature outside [0, F) does not split.
struct Rule {
  bool splits, first_right;
  int64_t f;
  int32_t thr;
};
MP4X_GBDT_HD Rule rule(int32_t feature, int32_t threshold, int32_t first_right, int64_t F) {
  Rule r;
  r.splits = feature >= 0 && (int64_t)feature < F;
  r.f = r.splits ? (int64_t)feature : 0;
  r.thr = threshold;
  r.first_right = first_right != 0;
  return r;
}
// 0: dropped, 1: first, 2: second.  bin < 0: no row (slot past the end, row index out of range).
MP4X_GBDT_HD int side(const Rule& r, int bin) {
  if (!r.splits || bin < 0) return 0;
  const bool right = bin > r.thr;
  return right == r.first_right ? 1 : 2;
}

MP4X_GBDT_HD int first_step(int wave) { return wave * kWaveSteps; }
MP4X_GBDT_HD int64_t slot_of(const gm::Tile& t, int step, int lane) {
  return (int64_t)t.lo + (int64_t)step * gm::kWave + lane;
}
MP4X_GBDT_HD int bits(uint64_t mask) { return __builtin_popcountll(mask); }
MP4X_GBDT_HD int rank_in_step(uint64_t mask, int lane) { return bits(mask & (((uint64_t)1 << lane) - 1)); }
// base: the tile's first or second base; before: the bits of the tile's earlier steps.
MP4X_GBDT_HD int64_t dest(int64_t base, int before, uint64_t mask, int lane) {
  return base + before + rank_in_step(mask, lane);
}
MP4X_GBDT_HD bool writable(int64_t d, int64_t m) { return d >= 0 && d < m; }
MP4X_GBDT_HD int64_t scan_index(int32_t T, int64_t tiles) { return gm::max64(0, gm::min64((int64_t)T, tiles)); }

}  // namespace gbdt_part
}  // namespace mp4x
