// The tile map of the grouped expert GEMM (K12): everything that turns a segment table into loop
// bounds and row ranges.  Plain C++ (no HIP types), the same code on the host and on the device:
// csrc/kernels/test_moe_gemm_map.cpp walks it on the CPU for every block id of every grid the
// launchers would build.  A kernel for the grouped GEMM reads a table through this header only.
//
// The table (int64, device memory in a launch):
//   ragged: offsets[G + 1] over rows [R, width].  Group g owns [c[g], c[g+1]) with c[0] = 0 and
//           c[g+1] = max(c[g], min(offsets[g+1], R)); offsets[0] is ignored.  Negative, non-monotone
//           and too-large entries are legal input.  The tail [c[G], R) is nobody's.
//   padded: valid[G * B] over rows [G, B * S, width].  Segment s = g * B + b owns the first
//           n(s) = max(0, min(valid[s], S)) rows of [s * S, (s + 1) * S); the rest is nobody's.
// (mp4x.parallel.moe._table_segments is the same rule in Python.)
//
// Invariants (asserted by the stand-alone test for every table it holds):
//   I1  every loop here has a trip count bounded by host-known numbers alone: forward_item and
//       wgrad_walk_init at most G + 1 trips, wgrad_next at most B + 1 trips a call, and a group's
//       walk yields at most wgrad_max_steps(layout, R, B, S, BK) steps;
//   I2  every row index handed out is in [0, R), and first + compute + zero <= R;
//   I3  over the row tiles [0, row_tiles) the owned rows are covered exactly once by `compute` (with
//       their own group) and the rows nobody owns exactly once by `zero`;
//   I4  all row arithmetic is int64; a raw table entry is only ever compared, never added to.
// Every table entry is read once into a local, clamped, then used.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_MAP_HD __host__ __device__ inline
#else
#define MP4X_MAP_HD inline
#endif

namespace mp4x {
namespace gemm_map {

constexpr int kRagged = 0;
constexpr int kPadded = 1;

MP4X_MAP_HD int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
MP4X_MAP_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
MP4X_MAP_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// Row tiles of the forward grid, from host-known numbers only.  Ragged: the G + 1 segments (the
// groups and the tail) sum to R rows, and sum ceil(L_i / BM) <= ceil(R / BM) + G.
MP4X_MAP_HD int64_t row_tiles(int layout, int64_t R, int64_t G, int64_t B, int64_t S, int64_t BM) {
  return layout == kRagged ? ceil_div(R, BM) + G : G * B * ceil_div(S, BM);
}

// What one row tile of the forward grid does: rows [first, first + compute) are group `group`'s and
// are computed, rows [first + compute, first + compute + zero) are nobody's and get +0.  Both 0: an
// empty item (the block returns before its first barrier).  `trips`: loop trips spent (I1).
struct Item {
  int64_t group, first, compute, zero, trips;
};

MP4X_MAP_HD Item forward_item(int layout, const int64_t* table, int64_t R, int64_t G, int64_t B, int64_t S,
                              int64_t BM, int64_t tile) {
  Item it = {0, 0, 0, 0, 0};
  if (tile < 0) return it;
  if (layout == kRagged) {
    int64_t lo = 0, t = tile;
    for (int64_t g = 0; g <= G; ++g) {                       // G + 1 trips at most
      it.trips = g + 1;
      int64_t hi = R;                                        // segment G is the tail
      if (g < G) {
        const int64_t raw = table[g + 1];
        hi = max64(lo, min64(raw, R));
      }
      const int64_t nt = ceil_div(hi - lo, BM);
      if (t < nt) {
        it.first = lo + t * BM;
        const int64_t rows = min64(BM, hi - it.first);
        it.group = g < G ? g : 0;
        it.compute = g < G ? rows : 0;
        it.zero = g < G ? 0 : rows;
        return it;
      }
      t -= nt;
      lo = hi;
    }
    return it;
  }
  const int64_t tps = ceil_div(S, BM);
  const int64_t seg = tile / tps, off = (tile % tps) * BM;
  it.trips = 1;
  if (seg >= G * B) return it;
  const int64_t raw = table[seg];
  const int64_t n = max64(0, min64(raw, S));
  const int64_t rows = min64(BM, S - off);
  it.group = seg / B;
  it.first = seg * S + off;
  it.compute = max64(0, min64(n - off, rows));
  it.zero = rows - it.compute;
  return it;
}

// The weight gradient: the (first row, count) pieces of group g in row order, cut into steps of at
// most BK rows.  Ragged: one piece; padded: B pieces.
struct Walk {
  int64_t piece, pieces, first, count, off, trips;
};

MP4X_MAP_HD int64_t wgrad_max_steps(int layout, int64_t R, int64_t B, int64_t S, int64_t BK) {
  return layout == kRagged ? ceil_div(R, BK) : B * ceil_div(S, BK);
}

MP4X_MAP_HD Walk wgrad_walk_init(int layout, const int64_t* table, int64_t R, int64_t G, int64_t B,
                                 int64_t g) {
  Walk w = {0, 0, 0, 0, 0, 0};
  if (g < 0 || g >= G) return w;
  if (layout == kRagged) {
    int64_t lo = 0, hi = 0;
    for (int64_t i = 0; i <= g; ++i) {                       // g + 1 <= G trips
      w.trips = i + 1;
      const int64_t raw = table[i + 1];
      lo = hi;
      hi = max64(lo, min64(raw, R));
    }
    w.pieces = 1;
    w.first = lo;
    w.count = hi - lo;
    return w;
  }
  w.piece = -1;                                              // wgrad_next loads piece 0 first
  w.pieces = B;
  return w;
}

// The next step of group g's walk: rows [row0, row0 + nrows), 1 <= nrows <= BK; false when done.
MP4X_MAP_HD bool wgrad_next(int layout, const int64_t* table, int64_t B, int64_t S, int64_t g, int64_t BK, Walk& w,
                            int64_t& row0, int64_t& nrows) {
  const int64_t max_trips = layout == kPadded ? B + 1 : 2;
  for (int64_t trip = 0; trip < max_trips; ++trip) {         // B + 1 trips at most (ragged: 2)
    w.trips = trip + 1;
    if (w.piece >= 0 && w.piece < w.pieces && w.off < w.count) {
      row0 = w.first + w.off;
      nrows = min64(BK, w.count - w.off);
      w.off += nrows;
      return true;
    }
    if (w.piece + 1 >= w.pieces) {
      w.piece = w.pieces;
      return false;
    }
    w.piece += 1;
    w.off = 0;
    if (layout == kPadded) {
      const int64_t seg = g * B + w.piece;
      const int64_t raw = table[seg];
      w.first = seg * S;
      w.count = max64(0, min64(raw, S));
    } else {
      w.count = 0;                                           // (a ragged walk has its one piece from init)
    }
  }
  return false;
}

}  // namespace gemm_map
}  // namespace mp4x
