// The row rule of the gated expert activation (K14; no kernel is in the tree): which
// rows of a segment table somebody owns, and which lane of which wave visits which (row, item).
// Plain C++ (no HIP types), the same code on the host and on the device:
// csrc/kernels/test_moe_act_map.cpp walks it on the CPU for every wave and lane of the grids a
// launcher would build.  A kernel for the activation reads a table through this header only.
//
// The table is moe_gemm_map.hpp's (int64, device memory in a launch):
//   ragged: offsets[G + 1] over rows [R, width].  Row r is owned iff r < c[G], with c[0] = 0 and
//           c[g+1] = max(c[g], min(offsets[g+1], R)); offsets[0] is ignored.  The recurrence is a
//           running maximum, so c[G] = max(0, max_g min(offsets[g+1], R)): every lane folds a stride
//           of the entries (ragged_end_part) and the wave joins the parts with max (exact, any order).
//   padded: valid[G * B] over rows [G, B * S, width].  Row r is owned iff
//           r % S < max(0, min(valid[r / S], S)).
// Negative, non-monotone and too-large entries are legal input.
//
// The walk: a row is `lanes` lanes wide (a power of two, 1 .. 64), a wave holds rows = 64 / lanes
// rows at a time and takes the row blocks wave, wave + nwaves, ...; lane sub of a row visits the
// items sub, sub + lanes, ... of its nitems (16-byte vectors or single elements).
//
// Invariants (asserted by the stand-alone test for every table it holds):
//   J1  every loop has a trip count bounded by host-known numbers alone: ragged_end_part at most
//       ceil(G / 64) <= kMaxGroups / 64 trips, a wave at most ceil(R / (rows * nwaves)) row blocks, a
//       lane at most ceil(nitems / lanes) items a row;
//   J2  every row index handed out is in [0, R) and every table index in [0, G + 1) or [0, G * B);
//   J3  every (row, item) pair is visited exactly once, and `owned` is the rule above;
//   J4  a raw table entry is read once into a local, clamped and only compared; the row arithmetic
//       is 32-bit on rows the launcher holds below 2^31 (one 32-bit division a row, none an item).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_ACT_HD __host__ __device__ inline
#else
#define MP4X_ACT_HD inline
#endif

namespace mp4x {
namespace act_map {

constexpr int kRagged = 0;
constexpr int kPadded = 1;
constexpr int kWave = 64;
constexpr int kItems = 4;                  // items a lane keeps in flight
constexpr int64_t kMaxGroups = 4096;       // ragged G: 64 lanes x 64 trips of the fold
constexpr int64_t kMaxRows = (int64_t)1 << 31;   // R < this: row indices are 32-bit

MP4X_ACT_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
MP4X_ACT_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// Lanes per row: the smallest power of two that leaves a lane at most kItems items, 64 at the most.
struct Shape {
  int lanes, lg, rows;
};
MP4X_ACT_HD Shape shape(int64_t nitems) {
  Shape s = {1, 0, kWave};
  while (s.lanes < kWave && (int64_t)s.lanes * kItems < nitems) {
    s.lanes <<= 1;
    ++s.lg;
  }
  s.rows = kWave >> s.lg;
  return s;
}

// Row blocks of `rows` rows, one wave each per round: what the launcher sizes its grid by.
MP4X_ACT_HD int64_t row_blocks(int64_t R, int rows) { return (R + rows - 1) / rows; }

// A lane's part of c[G]: the maximum of min(offsets[g + 1], R) over g = lane, lane + 64, ..., and 0.
MP4X_ACT_HD int64_t ragged_end_part(const int64_t* table, int64_t G, int64_t R, int lane, int64_t& trips) {
  int64_t m = 0;
  trips = 0;
  for (int64_t g = lane; g < G; g += kWave) {
    ++trips;
    const int64_t raw = table[g + 1];
    m = max64(m, min64(raw, R));
  }
  return m;
}
MP4X_ACT_HD int64_t ragged_end_join(int64_t a, int64_t b) { return max64(a, b); }

// Whether somebody owns row r < R of a padded table (S >= 1, R = G * B * S < 2^31); `seg` is the
// table entry read.
MP4X_ACT_HD bool padded_owned(const int64_t* table, uint32_t r, uint32_t S, uint32_t& seg) {
  seg = r / S;
  const int64_t raw = table[seg];
  const int64_t n = max64(0, min64(raw, (int64_t)S));
  return (int64_t)(r - seg * S) < n;
}

// The row of `lane` in the row block that starts at r0, or -1 past R; `sub` is the lane's first item.
MP4X_ACT_HD int64_t lane_row(const Shape& s, int64_t r0, int64_t R, int lane, int& sub) {
  sub = lane & (s.lanes - 1);
  const int64_t r = r0 + (lane >> s.lg);
  return r < R ? r : -1;
}

}  // namespace act_map
}  // namespace mp4x
