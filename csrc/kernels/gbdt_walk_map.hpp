// Chunk plan and step rule of the GBDT forest walk (K18, gbdt_predict.hip).  Plain C++ (no HIP types),
// the same code on the host and on the device: csrc/kernels/test_gbdt_walk_map.cpp walks it on the CPU.
// The kernel reads `tree_off` and forms every node, value and bin index through this header only.
//
// The forest: nodes int32[N, 4] = (feature, threshold, left, right), children relative to the tree's
// first node; value f64[N]; tree_off int32[T + 1].  Any bits are legal input.  Tree t owns the nodes
// [o[t], o[t+1]) with o[0] = 0 and o[t+1] = max(o[t], min(tree_off[t+1], N)) (clamp_off; tree_off[0] is
// ignored), so 0 <= o[t] <= o[t+1] <= N whatever the table holds.
//
// A row's walk in a tree of `size` > 0 nodes starts at node 0 and takes `steps` steps (step): at an
// inner node (0 <= feature < F and both children in [0, size)) it moves right iff bin > threshold,
// else left; at any other node it stays.  So the node index stays in [0, size) by induction, the
// feature a bin is read at (bin_feature) is in [0, F), and neither a cycle nor a child out of range
// nor a feature >= F can lengthen a loop or form an address out of range.
//
// Chunks (next_chunk): a chunk is a run of consecutive trees, at most kChunkTrees of them, whose
// nodes together fit kChunkNodes; it is staged in LDS (16-byte node records and 8-byte values side by
// side) and walked from there.  A single tree larger than kChunkNodes is its own chunk (`big`) and is
// walked from global memory with the same step.  The plan is greedy from tree 0 and a function of
// (tree_off, T, N) alone, so every block finds the same chunks.  Every chunk holds at least one tree:
// the chunk loop has at most T trips.
//
// Rows: a block owns a tile of kRowTile = kBlock * kRowsPerLane consecutive rows; thread `tid` owns the
// rows tile + u * kBlock + tid, u < kRowsPerLane (consecutive lanes, consecutive rows), walks them
// interleaved and keeps their float64 sums in registers over all chunks.  shape(F) says where the
// bins of a tile are read from: an LDS copy with a row stride of stride_dw(F) dwords - odd, so the 64
// lanes that read one feature of 64 consecutive rows hit 64 distinct banks - when kRowTile rows fit
// kRowTileBytes, else global memory.  The smallest F that takes the global form is kGlobalF = 45.
//
// Invariants (asserted by the stand-alone test for every forest it holds):
//   W1  every loop has a host-known trip count: at most T chunks, at most kChunkTrees trees a chunk,
//       exactly `steps` <= kMaxSteps steps a tree;
//   W2  the chunks are disjoint, consecutive and cover every tree once; a chunk that is not big has at
//       most kChunkNodes nodes;
//   W3  every node, value, bin and tile-byte index formed is in range;
//   W4  the result equals a direct evaluation of the definition.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_WALK_HD __host__ __device__ inline
#else
#define MP4X_WALK_HD inline
#endif

namespace mp4x {
namespace gbdt_walk {

constexpr int kMaxSteps = 64;                    // steps: the longest root-to-leaf path, in edges
constexpr int kBlock = 256;                      // threads a block
constexpr int kRowsPerLane = 4;                  // rows whose walks a lane interleaves
constexpr int kRowTile = kBlock * kRowsPerLane;  // rows a block
constexpr int kChunkNodes = 512;                 // nodes of a chunk in LDS: 16 + 8 bytes a node
constexpr int kChunkTrees = 64;                  // trees a chunk at most: one window of tree_off
constexpr int kChunkBytes = kChunkNodes * 24 + 2 * kChunkTrees * 4;   // nodes | values | two windows
constexpr int kRowTileBytes = 45056;             // the bins of a tile in LDS, at most
constexpr int kGlobalF = 45;                     // the smallest F whose bins are read from global memory
constexpr int64_t kMaxRows = (int64_t)1 << 31;   // n, N below this

struct Node {
  int32_t feature, threshold, left, right;
};

MP4X_WALK_HD int32_t clamp_off(int32_t raw, int32_t lo, int32_t N) {
  const int32_t hi = raw < N ? raw : N;
  return hi > lo ? hi : lo;
}

MP4X_WALK_HD bool is_inner(const Node& nd, int32_t size, int64_t F) {
  return nd.feature >= 0 && (int64_t)nd.feature < F && nd.left >= 0 && nd.left < size && nd.right >= 0 && nd.right < size;
}
// The column the walk reads a row's bin at: the node's feature at an inner node, else column 0 (F >= 1).
MP4X_WALK_HD int64_t bin_feature(const Node& nd, int32_t size, int64_t F) {
  return is_inner(nd, size, F) ? (int64_t)nd.feature : 0;
}
// The next node of a row that stands on `nd` with `bin` at bin_feature; -1: the row stays.
MP4X_WALK_HD int32_t step(const Node& nd, int32_t size, int64_t F, int bin) {
  if (!is_inner(nd, size, F)) return -1;
  return bin > nd.threshold ? nd.right : nd.left;
}

// The chunk that starts at a tree whose first node is o0: raw[i] = tree_off[t0 + 1 + i] for i < avail,
// avail = min(kChunkTrees, T - t0) >= 1.
struct Chunk {
  int trees;        // >= 1
  int32_t nodes;    // o[t0 + trees] - o0
  bool big;         // one tree larger than kChunkNodes: walked from global memory
};
MP4X_WALK_HD Chunk next_chunk(const int32_t* raw, int avail, int32_t o0, int32_t N) {
  Chunk c = {0, 0, false};
  int32_t lo = o0;
  for (int i = 0; i < avail && i < kChunkTrees; ++i) {
    const int32_t hi = clamp_off(raw[i], lo, N);
    if (hi - o0 > kChunkNodes) break;
    lo = hi;
    ++c.trees;
  }
  if (c.trees == 0) {
    c.trees = 1;
    c.big = true;
    lo = clamp_off(raw[0], o0, N);
  }
  c.nodes = lo - o0;
  return c;
}
MP4X_WALK_HD int window(int64_t T, int64_t t0) { return (int)(T - t0 < kChunkTrees ? T - t0 : kChunkTrees); }

// Where the bins of a tile are read from.
struct Shape {
  bool lds;
  int stride;       // bytes a row of the LDS tile
};
MP4X_WALK_HD int64_t stride_dw(int64_t F) { return ((F + 3) / 4) | 1; }
MP4X_WALK_HD Shape shape(int64_t F) {
  Shape s = {false, 0};
  if (F < kGlobalF) {
    s.lds = true;
    s.stride = (int)stride_dw(F) * 4;
  }
  return s;
}
static_assert(((kGlobalF - 1 + 3) / 4 | 1) * 4 * kRowTile <= kRowTileBytes && ((kGlobalF + 3) / 4 | 1) * 4 * kRowTile > kRowTileBytes,
              "kGlobalF is the smallest F whose tile does not fit");
static_assert(kChunkBytes + kRowTileBytes <= 65536, "a block's LDS");

// The rows of a block's tile and the row a thread owns in it (clamped to the tile's last row: a lane
// past the end walks that row and stores nothing).
MP4X_WALK_HD int64_t tile_rows(int64_t n, int64_t block) {
  const int64_t left = n - block * kRowTile;
  return left < kRowTile ? left : kRowTile;
}
MP4X_WALK_HD int lane_row(int tid, int u) { return u * kBlock + tid; }

// Staging of a tile's bytes [a0, a1) (addresses): 16-byte loads cover [head_end, tail_begin), byte loads
// the rest.  A range that holds no aligned 16 bytes is all head.
struct Span {
  uint64_t head_end, tail_begin;
};
MP4X_WALK_HD Span span16(uint64_t a0, uint64_t a1) {
  Span s;
  s.head_end = (a0 + 15) & ~(uint64_t)15;
  s.tail_begin = a1 & ~(uint64_t)15;
  if (s.head_end >= s.tail_begin) s.head_end = s.tail_begin = a1;
  return s;
}
// The LDS byte of byte `i` of a tile's contiguous global range.
MP4X_WALK_HD int tile_byte(int i, int F, int stride) { return (i / F) * stride + i % F; }

}  // namespace gbdt_walk
}  // namespace mp4x
