// K19 — GBDT feature binning on the GPU: float features to byte bins by a fixed binary search (gfx950).
//
//   bins[r, f] = missing if X[r, f] is NaN, else the position the search of gbdt_bin_map.hpp ends on
//
// 4 (or 2) bytes in and 1 byte out an element, and between them a dependent chain of `steps` table reads.
//
//   k_gbdt_bin   a block of kBlock = 1024 threads serves the tile of kRowTile = 4096 consecutive rows of one
//                group of up to 64 consecutive features.  blockIdx = tile * groups + group: the blocks of
//                a tile's groups run side by side and read neighbouring 256-byte pieces of the same rows.
//                Table: the group's keys stand in LDS transposed, entry e of feature fl at e * 64 + fl,
//                kNever from the clamped cnt on, 2**steps - 1 entries a feature (dynamic LDS: 65280 bytes
//                at E = 255, two blocks a CU; 16128 at E = 63).  It is staged in squares of 8 edges x 8
//                features: a wave reads 8 runs of 32 bytes and writes 8 banks, neither 64 lines nor one
//                bank.  One barrier; 16 waves share the table, so staging (at most 65280 bytes from L2)
//                is at most 5.0 % of the tile's 4096 * 64 * 5 bytes.
//                Lanes: a lane owns one feature for the whole tile, lane = sub * W + fl with W the group's
//                width and sub < R = 64 / W: a wave takes R rows at a time (one row of 64 features as one
//                256-byte load when W = 64; R * W adjacent elements when F < 64; lanes from R * W on
//                idle).  Since the feature is fixed, the entries of the first two steps - one and two
//                values a lane - are read once into registers; the steps from the third on are one
//                ds_read_b32, one unsigned compare and one select each.  Lanes of one feature and
//                different rows (F < 64) share a bank and can conflict R ways.
//                Rows: a wave issues the loads of kRowsInFlight = 4 batches (waves apart, so the block
//                reads consecutive rows), then interleaves their four searches, then stores: a wave
//                instruction writes the adjacent bytes of its rows.  No alignment of a row is assumed.
//
// No atomics, no scratch, no block waits on another; no allocation and no host read: one launch,
// recordable in a graph.  Integer compares only (gbdt_bin_map.hpp), so no float mode matters; float16 and
// bfloat16 are widened exactly (a float16 denormal is a float32 normal).
#include "common.hpp"
#include "gbdt_bin_map.hpp"

namespace mp4x {

namespace gb = gbdt_bin;

template <int DT>
__global__ __launch_bounds__(gb::kBlock) void k_gbdt_bin(const typename Elem<DT>::S* __restrict__ X,
                                                         const uint32_t* __restrict__ edges,
                                                         const int32_t* __restrict__ cnt, int64_t n, int64_t F, int E,
                                                         int steps, int groups, int missing,
                                                         uint8_t* __restrict__ bins) {
  extern __shared__ uint32_t tab[];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x / groups, f0 = (int64_t)(blockIdx.x % groups) * gb::kGroup;
  const int W = (int)(F - f0 < gb::kGroup ? F - f0 : gb::kGroup);
  const int trows = gb::table_rows(steps);

  // squares of 8 entries x 8 features: square q covers the features (q % 8) * 8 .. + 7 and the entries
  // (q / 8) * 8 .. + 7; lane l of it the feature l / 8 and the entry l % 8 of those
  for (int j = tid; j < ((trows + 7) / 8) * 8 * gb::kGroup; j += gb::kBlock) {
    const int q = j >> 6, l = j & 63;
    const int fl = (q & 7) * 8 + (l >> 3), e = (q >> 3) * 8 + (l & 7);
    if (e >= trows) continue;
    uint32_t k = gb::kNever;
    if (fl < W) {
      const int32_t raw = cnt[f0 + fl];
      const int c = raw < 0 ? 0 : raw > E ? E : raw;
      if (e < c) k = gb::edge_key(edges[(f0 + fl) * E + e]);
    }
    tab[e * gb::kGroup + fl] = k;
  }
  __syncthreads();

  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int R = gb::kGroup / W, sub = lane / W, fl = lane - sub * W;   // fl < W; sub >= R: an idle lane
  const int top = steps ? 1 << (steps - 1) : 0, half = top >> 1;      // the first two steps (0: there is none)
  const uint32_t e0 = top ? tab[(top - 1) * gb::kGroup + fl] : gb::kNever;
  const uint32_t e1lo = half ? tab[(half - 1) * gb::kGroup + fl] : gb::kNever;
  const uint32_t e1hi = half ? tab[(top + half - 1) * gb::kGroup + fl] : gb::kNever;

  const int64_t row0 = tile * gb::kRowTile;
  const int rows = (int)(n - row0 < gb::kRowTile ? n - row0 : gb::kRowTile);   // >= 1 by the grid
  const int batches = (rows + R - 1) / R;
  for (int b0 = wave; b0 < batches; b0 += gb::kWaves * gb::kRowsInFlight) {
    int64_t at[gb::kRowsInFlight];
    bool on[gb::kRowsInFlight];
    typename Elem<DT>::S raw[gb::kRowsInFlight];
    uint32_t xk[gb::kRowsInFlight];
    int pos[gb::kRowsInFlight];
#pragma unroll
    for (int u = 0; u < gb::kRowsInFlight; ++u) {
      const int lr = (b0 + u * gb::kWaves) * R + sub;
      on[u] = sub < R && lr < rows;
      at[u] = (row0 + lr) * F + f0 + fl;
      raw[u] = 0;
      if (on[u]) raw[u] = X[at[u]];
    }
    bool nan[gb::kRowsInFlight];
#pragma unroll
    for (int u = 0; u < gb::kRowsInFlight; ++u) {
      const uint32_t bits = __float_as_uint(Elem<DT>::load(raw[u]));
      nan[u] = gb::is_nan(bits);
      xk[u] = gb::key(bits);
      pos[u] = gb::step(0, top, e0, xk[u]);
      pos[u] = gb::step(pos[u], half, pos[u] ? e1hi : e1lo, xk[u]);
    }
    for (int s = half >> 1; s; s >>= 1) {
      uint32_t entry[gb::kRowsInFlight];
#pragma unroll
      for (int u = 0; u < gb::kRowsInFlight; ++u) {
        MP4X_DASSERT(pos[u] + s - 1 >= 0 && pos[u] + s - 1 < trows);
        entry[u] = tab[(pos[u] + s - 1) * gb::kGroup + fl];
      }
#pragma unroll
      for (int u = 0; u < gb::kRowsInFlight; ++u) pos[u] = gb::step(pos[u], s, entry[u], xk[u]);
    }
#pragma unroll
    for (int u = 0; u < gb::kRowsInFlight; ++u)
      if (on[u]) bins[at[u]] = (uint8_t)(nan[u] ? missing : pos[u]);
  }
}

}  // namespace mp4x

using namespace mp4x;

extern "C" int mp4x_gbdt_bin(const void* X, int dtype, const float* edges, const int32_t* cnt, int64_t n, int64_t F,
                             int E, int missing, uint8_t* bins, void* stream) {
  if (n < 0 || n >= gb::kMaxRows || F < 0 || F >= gb::kMaxRows || E < 0 || E > gb::kMaxEdges || missing < 0 ||
      missing > 255 || (dtype != MP4X_F32 && dtype != MP4X_F16 && dtype != MP4X_BF16))
    return MP4X_E_BADARG;
  if (n == 0 || F == 0) return 0;
  const int64_t groups = (F + gb::kGroup - 1) / gb::kGroup, tiles = (n + gb::kRowTile - 1) / gb::kRowTile;
  if (groups * tiles >= gb::kMaxRows) return MP4X_E_BADARG;
  if (!X || ((uintptr_t)X & (dtype == MP4X_F32 ? 3 : 1)) || !bins || !cnt || ((uintptr_t)cnt & 3) ||
      (E && (!edges || ((uintptr_t)edges & 3))))
    return MP4X_E_BADARG;
  const int steps = gb::steps_for(E);
  const dim3 grid((unsigned)(groups * tiles));
  const size_t lds = (size_t)gb::lds_bytes(steps);
  auto launch = [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    hipLaunchKernelGGL(k_gbdt_bin<DT>, grid, dim3(gb::kBlock), lds, (hipStream_t)stream,
                       (const typename Elem<DT>::S*)X, (const uint32_t*)edges, cnt, n, F, E, steps, (int)groups, missing,
                       bins);
    return (int)hipGetLastError();
  };
  if (dtype == MP4X_F32) return launch(IntC<MP4X_F32>{});
  if (dtype == MP4X_F16) return launch(IntC<MP4X_F16>{});
  return launch(IntC<MP4X_BF16>{});
}
