// Limits, shapes and the search step of the GBDT feature binning (K19, gbdt_bin.hip).  Plain C++ (no HIP
// types), the same code on the host and on the device.
//
// The definition: with c = clamp(cnt[f], 0, E) and x = X[r, f] widened to float32,
//
//   pos = 0
//   for s in (128, 64, 32, 16, 8, 4, 2, 1):
//     if pos + s <= c and edges[f, pos + s - 1] <= x: pos += s       (IEEE: denormals count, -0 == +0,
//   bin = missing if x is NaN else pos                                a NaN edge is never <= x)
//
// Keys.  The compare is done on order-preserving unsigned keys of the float32 bits (key), so it does not
// depend on the compile's float32 denormal mode: -0.0 takes the key of +0.0, a negative value the
// complement of its bits, any other value its bits with the sign bit set.  For two non-NaN floats a, b:
// a <= b iff key(a) <= key(b).  The largest key of a non-NaN value is key(+inf) = 0xff800000; an edge that
// is NaN takes kNever = 0xffffffff (edge_key), which no key of a non-NaN x reaches: it is never <= x.
//
// The table.  steps_for(E) = ceil(log2(E + 1)) is the number of steps that can move: a step s >= 2**steps
// has s > E >= c and never does.  The table of a feature holds 2**steps - 1 keys, edge_key of edges[f, e]
// for e < c and kNever from there on.  Then
//
//   pos = 0
//   for s in (2**(steps - 1), ..., 2, 1): if table[pos + s - 1] <= key(x): pos += s
//
// equals the definition: before the step s, pos is a multiple of 2 s and pos <= 2**steps - 2 s (induction:
// every earlier step added 0 or its own s' = a multiple of 2 s, and the sum of all earlier s' is 2**steps
// - 2 s), so the entry read, pos + s - 1 <= 2**steps - s - 1 <= 2**steps - 2, is in the table whatever it
// holds.  Where pos + s <= c it is the edge the definition compares; where pos + s > c it is kNever and the
// step does not move, as the definition's own test says.  No index is formed from anything but pos.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_BIN_HD __host__ __device__ inline
#else
#define MP4X_BIN_HD inline
#endif

namespace mp4x {
namespace gbdt_bin {

constexpr int kMaxEdges = 255;                   // E: a bin is a byte
constexpr int kGroup = 64;                       // features a block serves: one a lane
constexpr int kBlock = 1024;                     // threads a block: 16 waves share one staged table
constexpr int kWaves = kBlock / 64;
constexpr int kRowsInFlight = 4;                 // row batches a wave loads before it searches them
constexpr int kRowTile = 4096;                   // rows a block
constexpr int64_t kMaxRows = (int64_t)1 << 31;   // n, F and the grid below this
constexpr uint32_t kNever = 0xffffffffu;         // the key of a NaN edge and of the fill past c

MP4X_BIN_HD bool is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
// The key of a non-NaN float32 by its bits.
MP4X_BIN_HD uint32_t key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0;             // -0.0 == +0.0
  return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
MP4X_BIN_HD uint32_t edge_key(uint32_t bits) { return is_nan(bits) ? kNever : key(bits); }
// One step of the search: the position after the step s, `entry` being table[pos + s - 1].
MP4X_BIN_HD int step(int pos, int s, uint32_t entry, uint32_t xkey) { return entry <= xkey ? pos + s : pos; }

MP4X_BIN_HD int steps_for(int E) {
  int steps = 0;
  while ((1 << steps) <= E) ++steps;
  return steps;
}
MP4X_BIN_HD int table_rows(int steps) { return (1 << steps) - 1; }
// The table of a block, transposed: entry e of the group's feature fl stands at e * kGroup + fl, so the
// 64 lanes of a wave (lane = feature) read 64 different banks whatever their positions are.
MP4X_BIN_HD int lds_bytes(int steps) { return table_rows(steps) * kGroup * 4; }
static_assert(((1 << 8) - 1) * kGroup * 4 <= 65536 && (1 << 8) > kMaxEdges, "the table of kMaxEdges edges fits a block's LDS");

}  // namespace gbdt_bin
}  // namespace mp4x
