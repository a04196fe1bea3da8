// Tile map of the GBDT histogram (K16, gbdt.hip): segment table -> which block owns which row slots
// of which node and which features, and which lane of the block visits which (row slot, feature).
// Plain C++ (no HIP types), the same code on the host and on the device:
// csrc/kernels/test_gbdt_hist_map.cpp walks it on the CPU for every block id and lane of the grid a
// launch builds.  The kernels read `seg` and index `rows` through this header only.
//
// The table is moe_gemm_map.hpp's ragged one: seg int64[k + 1] over the m row slots of `rows`.  Node j
// owns the slots [c[j], c[j+1]) with c[0] = 0 and c[j+1] = max(c[j], min(seg[j+1], m)); seg[0] is
// ignored.  Negative, non-monotone and too-large entries are legal input: every entry is read once
// into a local, clamped and only then used.
//
// Tiles: node j's slots are cut into tiles_of(c[j+1] - c[j]) tiles of kTile slots; T[j] is the number
// of tiles of the nodes before j (T[k] the total).  build_tables writes c and T (int32: m < 2^31)
// in one sequential pass; on the device one lane runs it over an LDS copy of the table, once a
// launch.  The grid is max_tiles(m, k) * groups(F, fg) blocks, a host-known bound of T[k]: a sum of
// ceilings is at most floor(m / kTile) + k.  Block id -> (tile, group) with the group fastest, so the
// blocks that read the same rows run next to each other; tile t -> node by find_node, a binary search
// of T; a tile id >= T[k] owns nothing.
//
// Lanes: a group is fg features (a power of two, 1 .. 64, shape()); lane l of a wave takes feature
// l % fg of the group and row l / fg of the wave's step, so the lanes of a wave spread over features
// first.  A block of kWaves waves covers rows_per_step() slots a step.
//
// Invariants (asserted by the stand-alone test for every table it holds):
//   H1  every loop has a trip count bounded by host-known numbers: build_tables k trips, find_node
//       at most 13 (k <= kMaxNodes), a lane at most ceil(kTile / rows_per_step) slots;
//   H2  0 <= c[j] <= c[j+1] <= m, T is non-decreasing, T[k] <= max_tiles(m, k), every slot handed
//       out is in [c[j], c[j+1]) of the tile's node and every feature in [0, F);
//   H3  every owned (slot, feature) pair is visited exactly once over the whole grid, by a block
//       whose node is the slot's owner; nothing else is visited.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_GBDT_HD __host__ __device__ inline
#else
#define MP4X_GBDT_HD inline
#endif

namespace mp4x {
namespace gbdt_map {

constexpr int kWave = 64;
constexpr int kWaves = 4;                        // waves a block (kBlock / 64)
constexpr int kTile = 4096;                      // row slots a tile
constexpr int kMaxNodes = 4096;                  // k: the table fits one block's LDS
constexpr int kMaxBins = 256;                    // bins are bytes
constexpr int kMaxShift = 200;                   // |s|: float64(x) * 2**s stays exact for every float32 x
constexpr int kLdsBytes = 32768;                 // private histogram a block: fg * B * 16 bytes
constexpr int64_t kMaxRows = (int64_t)1 << 31;   // m, n < this: slots and rows are 32-bit

constexpr int32_t kQMax = 2147483647;            // a quantised value is clamped to +-kQMax

// The quantiser: rint(f64(x) * 2^s), half to even, NaN -> 0, clamped.  |s| <= kMaxShift: the product is exact.
MP4X_GBDT_HD int32_t q(float x, int s) {
  const double v = __builtin_rint(__builtin_ldexp((double)x, s));
  if (v != v) return 0;
  if (v >= (double)kQMax) return kQMax;
  if (v <= -(double)kQMax) return -kQMax;
  return (int32_t)v;
}

MP4X_GBDT_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
MP4X_GBDT_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// Features a group: the largest power of two whose [fg, B, 2] int64 histogram fits kLdsBytes (8 at
// B = 256, 64 at B <= 32), no more than the power of two that covers F.
struct Shape {
  int fg, lg, rows;       // features a group, log2, rows a wave step
};
MP4X_GBDT_HD Shape shape(int64_t F, int B) {
  Shape s = {1, 0, kWave};
  while (s.fg < kWave && s.fg < F && (int64_t)(2 * s.fg) * B * 16 <= kLdsBytes) {
    s.fg <<= 1;
    ++s.lg;
  }
  s.rows = kWave >> s.lg;
  return s;
}
MP4X_GBDT_HD int64_t groups(int64_t F, int fg) { return (F + fg - 1) / fg; }
MP4X_GBDT_HD int rows_per_step(const Shape& s) { return s.rows * kWaves; }

MP4X_GBDT_HD int64_t tiles_of(int64_t len) { return (len + kTile - 1) / kTile; }
MP4X_GBDT_HD int64_t max_tiles(int64_t m, int64_t k) { return m / kTile + k; }

// c[0 .. k] and T[0 .. k] from the raw table (k + 1 entries, entry 0 ignored).
MP4X_GBDT_HD void build_tables(const int64_t* seg, int64_t k, int64_t m, int32_t* c, int32_t* T) {
  int64_t prev = 0, tiles = 0;
  c[0] = 0;
  T[0] = 0;
  for (int64_t j = 0; j < k; ++j) {
    const int64_t raw = seg[j + 1];
    const int64_t hi = max64(prev, min64(raw, m));
    tiles += tiles_of(hi - prev);
    c[j + 1] = (int32_t)hi;
    T[j + 1] = (int32_t)tiles;
    prev = hi;
  }
}

// The node of tile t < T[k]: the largest j < k with T[j] <= t (then T[j+1] > t: the node has tiles).
MP4X_GBDT_HD int find_node(const int32_t* T, int k, int32_t t, int& trips) {
  int lo = 0, hi = k;       // T[lo] <= t < T[hi]
  trips = 0;
  while (hi - lo > 1) {
    ++trips;
    const int mid = (lo + hi) >> 1;
    if (T[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What a block owns: node, slots [lo, hi), features [f0, f1); `owns` false for a tile past T[k].
struct Tile {
  bool owns;
  int node;
  int32_t lo, hi;
  int f0, f1;
};
MP4X_GBDT_HD Tile tile_of(const int32_t* c, const int32_t* T, int k, int64_t block, int64_t ngroups, int64_t F,
                          const Shape& s) {
  Tile t = {false, 0, 0, 0, 0, 0};
  const int64_t tile = block / ngroups, grp = block - tile * ngroups;
  if (k < 1 || tile >= (int64_t)T[k]) return t;
  int trips;
  t.node = find_node(T, k, (int32_t)tile, trips);
  const int64_t lo = (int64_t)c[t.node] + (tile - T[t.node]) * kTile;
  t.lo = (int32_t)lo;
  t.hi = (int32_t)min64(lo + kTile, (int64_t)c[t.node + 1]);
  t.f0 = (int)(grp * s.fg);
  t.f1 = (int)min64((int64_t)t.f0 + s.fg, F);
  t.owns = t.lo < t.hi;
  return t;
}

// Thread `tid` of a block: its feature (-1: past the group's tail) and the offset of its first slot
// in the tile; it then takes every rows_per_step()-th slot.
MP4X_GBDT_HD int lane_feature(const Shape& s, const Tile& t, int tid) {
  const int f = t.f0 + (tid & (s.fg - 1));
  return f < t.f1 ? f : -1;
}
MP4X_GBDT_HD int lane_row(const Shape& s, int tid) { return (tid >> 6) * s.rows + ((tid & 63) >> s.lg); }

}  // namespace gbdt_map
}  // namespace mp4x
