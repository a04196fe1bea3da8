// Row tiles, keys and the step rule of the GBDT forest walk over float features (K20, gbdt_predict_float.hip).
// Plain C++ (no HIP types), the same code on the host and on the device.  The forest, the tree table, the
// chunk plan and `is_inner` are gbdt_walk_map.hpp's; the keys are gbdt_bin_map.hpp's.
//
// The forest: K18's records with the threshold replaced by a uint32 key K (kept as its int32 bits).  A row's
// value x, widened to float32, takes xkey(bits): key(bits) for a non-NaN x, kNanKey = 0xfffffffe for a NaN.
// At an inner node the row moves right iff K <= xkey, compared as unsigned (step); at any other node it
// stays.  key(+inf) = 0xff800000 is the largest key of a non-NaN value, so K = kNanKey sends only a NaN row
// right, K = 0xffffffff nobody and K = 0 everybody.
//
// Rows: a key is 4 bytes where K18's bin is 1, so the tile depends on F.  A block of kBlock threads owns
// kBlock * U consecutive rows, thread `tid` the rows tile + u * kBlock + tid, u < U, walked interleaved.
// rows_per_lane(F) is the largest U of 4, 2, 1 whose tile of keys, at a row stride of stride_dw(F) = F | 1
// dwords (odd: the 64 lanes that read one feature of 64 consecutive rows hit 64 banks), fits kTileBytes:
//
//   F <= 11: U = 4, 1024 rows     F <= 21: U = 2, 512 rows     F <= 43: U = 1, 256 rows
//
// and 0 from kGlobalF = 44 on: the keys do not fit, the walk reads X from global memory and forms the key
// per read, kGlobalRows = 4 rows a lane.  A block's dynamic LDS is the chunk plus its own tile (lds_bytes),
// not the largest one, so small F leaves room for more blocks on a CU.
#pragma once
#include "gbdt_bin_map.hpp"
#include "gbdt_walk_map.hpp"

namespace mp4x {
namespace gbdt_fwalk {

namespace gw = gbdt_walk;

constexpr int kTileBytes = gw::kRowTileBytes;    // the keys of a tile in LDS, at most
constexpr int kGlobalF = 44;                     // the smallest F whose rows are read from global memory
constexpr int kGlobalRows = 4;                   // rows a lane in the global form
constexpr uint32_t kNanKey = 0xfffffffeu;        // the key of a NaN row: above every non-NaN key

MP4X_WALK_HD uint32_t xkey(uint32_t bits) { return gbdt_bin::is_nan(bits) ? kNanKey : gbdt_bin::key(bits); }
// The next node of a row that stands on `nd` with the key `xk` at gw::bin_feature; -1: the row stays.
MP4X_WALK_HD int32_t step(const gw::Node& nd, int32_t size, int64_t F, uint32_t xk) {
  if (!gw::is_inner(nd, size, F)) return -1;
  return (uint32_t)nd.threshold <= xk ? nd.right : nd.left;
}

constexpr int64_t stride_dw(int64_t F) { return F | 1; }
// Rows a lane with the tile's keys in LDS; 0: they do not fit (the global form).
constexpr int rows_per_lane(int64_t F) {
  for (int U = 4; U >= 1; U >>= 1)
    if (stride_dw(F) * 4 * gw::kBlock * U <= kTileBytes) return U;
  return 0;
}
constexpr int tile_rows_of(int64_t F) { return gw::kBlock * (rows_per_lane(F) ? rows_per_lane(F) : kGlobalRows); }
constexpr int lds_bytes(int64_t F) {
  return gw::kChunkBytes + (rows_per_lane(F) ? (int)stride_dw(F) * 4 * gw::kBlock * rows_per_lane(F) : 0);
}
static_assert(rows_per_lane(1) == 4 && rows_per_lane(11) == 4 && rows_per_lane(12) == 2 && rows_per_lane(21) == 2 &&
                  rows_per_lane(22) == 1 && rows_per_lane(kGlobalF - 1) == 1 && rows_per_lane(kGlobalF) == 0,
              "the tile rule stated above; kGlobalF is the smallest F whose tile does not fit");
static_assert(rows_per_lane((int64_t)1 << 31) == 0 && gw::kChunkBytes + kTileBytes <= 65536, "a block's LDS");

// The rows of a block's tile of `tile` rows: >= 1 when the grid is ceil(n / tile).
MP4X_WALK_HD int64_t tile_rows(int64_t n, int64_t block, int tile) {
  const int64_t left = n - block * tile;
  return left < tile ? left : tile;
}

}  // namespace gbdt_fwalk
}  // namespace mp4x
