// K18 — GBDT forest prediction on the GPU: an LDS tree walk (gfx950).
//
//   pred[r] = init[r] (or +0.0) + sum over the trees t = 0 .. T-1, in that order, of value[o[t] + j(r, t)]
//   leaf[r, t] = j(r, t), the node the walk of row r in tree t ends on (-1 for a tree without nodes)
//
// with the tree table, the walk and the chunk plan of gbdt_walk_map.hpp.  One kernel, two
// instantiations (the bins of a tile in LDS, or read from global memory for F >= kGlobalF):
//
//   k_gbdt_predict   a block per tile of kRowTile = 1024 consecutive rows; a thread owns kRowsPerLane = 4
//                    of them (tile + u * 256 + tid) and keeps their float64 sums in registers from the
//                    first chunk to the last, so the sum's order is the tree order.
//                    Bins: the tile's bytes are one contiguous range of `bins`; 16-byte loads over its
//                    aligned middle and byte loads at the ragged head and tail scatter it into LDS rows
//                    of an odd number of dwords.
//                    Forest: the block walks the chunks in order.  A window of kChunkTrees raw offsets
//                    stands in LDS (two windows in turn: the next one is loaded while this chunk is
//                    staged); every thread runs next_chunk over it (LDS broadcast reads, no result to
//                    share), then the chunk's node records (int4) and values are staged with coalesced
//                    loads.  Per tree the four walks of a lane are interleaved: a step of a row is one
//                    16-byte LDS read of the node, one LDS byte read of the bin and a select, and the
//                    dependent chain of one row overlaps the three others.  The step loop has exactly
//                    `steps` trips; a wave leaves it when a ballot says no lane stands on an inner node.
//                    A tree larger than kChunkNodes is walked from global memory by the same code.
//                    Two barriers a chunk; no atomics, no scratch, no block waits on another.
//
// Only float64 additions, one a tree and row, in tree order: nothing to contract, no packed f32.  The
// compile's float64 denormal mode is IEEE (the AMDGPU default; only f32 flushing is an option), so
// denormal values and sums keep their bits.  No allocation, no host read: recordable in a graph.
#include "common.hpp"
#include "gbdt_walk_map.hpp"

namespace mp4x {

namespace gw = gbdt_walk;
static_assert(gw::kBlock == kBlock, "a block is kBlock threads");

// The walks of a lane's rows through one tree of `size` > 0 nodes at nd / val (LDS or global memory),
// and the tree's term of every sum.  BINS_LDS: row_at[u] is the row's byte offset in the LDS tile, else
// its byte offset in `gbins`.
template <bool BINS_LDS>
__device__ __forceinline__ void walk_tree(const int4* nd, const double* val, int32_t size, int64_t F, int steps,
                                          const uint8_t* tile, const uint8_t* __restrict__ gbins,
                                          const int64_t (&row_at)[gw::kRowsPerLane], int32_t (&j)[gw::kRowsPerLane],
                                          double (&acc)[gw::kRowsPerLane]) {
#pragma unroll
  for (int u = 0; u < gw::kRowsPerLane; ++u) j[u] = 0;
  for (int s = 0; s < steps; ++s) {
    gw::Node rec[gw::kRowsPerLane];
    int bin[gw::kRowsPerLane];
#pragma unroll
    for (int u = 0; u < gw::kRowsPerLane; ++u) {
      MP4X_DASSERT(j[u] >= 0 && j[u] < size);
      const int4 v = nd[j[u]];
      rec[u] = gw::Node{v.x, v.y, v.z, v.w};
    }
#pragma unroll
    for (int u = 0; u < gw::kRowsPerLane; ++u) {
      const int64_t f = gw::bin_feature(rec[u], size, F);
      bin[u] = BINS_LDS ? (int)tile[row_at[u] + f] : (int)gbins[row_at[u] + f];
    }
    bool moved = false;
#pragma unroll
    for (int u = 0; u < gw::kRowsPerLane; ++u) {
      const int32_t nx = gw::step(rec[u], size, F, bin[u]);
      moved |= nx >= 0;
      j[u] = nx >= 0 ? nx : j[u];
    }
    if (!__any(moved)) break;                            // wave-uniform: every lane stands on a non-inner node
  }
#pragma unroll
  for (int u = 0; u < gw::kRowsPerLane; ++u) acc[u] += val[j[u]];
}

template <bool BINS_LDS>
__global__ __launch_bounds__(kBlock) void k_gbdt_predict(const uint8_t* __restrict__ bins, const int4* __restrict__ nodes,
                                                         const double* __restrict__ value,
                                                         const int32_t* __restrict__ tree_off, const double* init,
                                                         int64_t n, int64_t F, int64_t T, int32_t N, int steps,
                                                         double* pred, int32_t* __restrict__ leaf) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int4* const s_nodes = (int4*)lds;
  double* const s_val = (double*)(lds + gw::kChunkNodes * 16);
  int32_t* const s_win = (int32_t*)(lds + gw::kChunkNodes * 24);      // [2][kChunkTrees]
  uint8_t* const s_bins = lds + gw::kChunkBytes;
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * gw::kRowTile;
  const int64_t rows = gw::tile_rows(n, blockIdx.x);     // >= 1: the grid is ceil(n / kRowTile)
  const gw::Shape sh = gw::shape(F);

  if (BINS_LDS) {                                        // the tile's bytes: one contiguous range of bins
    const uint8_t* src = bins + row0 * F;
    const int Fi = (int)F, bytes = (int)rows * Fi;       // F < kGlobalF: a tile's bytes fit an int
    const gw::Span sp = gw::span16((uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)src + (uint64_t)bytes);
    const int head = (int)(sp.head_end - (uint64_t)(uintptr_t)src), tail = (int)(sp.tail_begin - (uint64_t)(uintptr_t)src);
    for (int i = tid; i < head; i += kBlock) s_bins[gw::tile_byte(i, Fi, sh.stride)] = src[i];
    for (int i = tail + tid; i < bytes; i += kBlock) s_bins[gw::tile_byte(i, Fi, sh.stride)] = src[i];
    for (int i = head + tid * 16; i < tail; i += kBlock * 16) {
      const u32x4 v = *(const u32x4*)(src + i);
      int r = i / Fi, c = i - r * Fi;
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        s_bins[r * sh.stride + c] = (uint8_t)(v[b >> 2] >> ((b & 3) * 8));
        if (++c == Fi) {
          c = 0;
          ++r;
        }
      }
    }
  }

  int64_t row_at[gw::kRowsPerLane];
  bool live[gw::kRowsPerLane];
  double acc[gw::kRowsPerLane];
#pragma unroll
  for (int u = 0; u < gw::kRowsPerLane; ++u) {
    const int lr = gw::lane_row(tid, u);
    live[u] = lr < rows;
    const int64_t r = live[u] ? lr : rows - 1;
    row_at[u] = BINS_LDS ? r * sh.stride : (row0 + r) * F;
    acc[u] = live[u] && init ? init[row0 + lr] : 0.0;
  }

  if (T > 0 && tid < gw::window(T, 0)) s_win[tid] = tree_off[1 + tid];
  __syncthreads();                                       // the tile and the first window stand
  int32_t o0 = 0;
  int par = 0;
  for (int64_t t0 = 0; t0 < T;) {                        // at most T chunks: every chunk holds a tree
    const int32_t* win = s_win + par * gw::kChunkTrees;
    const gw::Chunk c = gw::next_chunk(win, gw::window(T, t0), o0, N);
    const int64_t t1 = t0 + c.trees;
    if (!c.big)
      for (int i = tid; i < c.nodes; i += kBlock) {
        s_nodes[i] = nodes[(int64_t)o0 + i];
        s_val[i] = value[(int64_t)o0 + i];
      }
    if (t1 < T && tid < gw::window(T, t1)) s_win[(par ^ 1) * gw::kChunkTrees + tid] = tree_off[t1 + 1 + tid];
    __syncthreads();
    int32_t lo = o0;
    for (int i = 0; i < c.trees; ++i) {
      const int32_t hi = gw::clamp_off(win[i], lo, N), size = hi - lo;
      int32_t j[gw::kRowsPerLane];
      if (size > 0) {
        if (c.big) walk_tree<BINS_LDS>(nodes + lo, value + lo, size, F, steps, s_bins, bins, row_at, j, acc);
        else walk_tree<BINS_LDS>(s_nodes + (lo - o0), s_val + (lo - o0), size, F, steps, s_bins, bins, row_at, j, acc);
      }
      if (leaf) {
#pragma unroll
        for (int u = 0; u < gw::kRowsPerLane; ++u)
          if (live[u]) leaf[(row0 + gw::lane_row(tid, u)) * T + t0 + i] = size > 0 ? j[u] : -1;
      }
      lo = hi;
    }
    __syncthreads();                                     // the chunk is read before the next one is staged
    o0 += c.nodes;
    t0 = t1;
    par ^= 1;
  }
#pragma unroll
  for (int u = 0; u < gw::kRowsPerLane; ++u)
    if (live[u]) pred[row0 + gw::lane_row(tid, u)] = acc[u];
}

}  // namespace mp4x

using namespace mp4x;

extern "C" int mp4x_gbdt_predict(const uint8_t* bins, const int32_t* nodes, const double* value, const int32_t* tree_off,
                                 const double* init, int64_t n, int64_t F, int64_t T, int64_t N, int steps, double* pred,
                                 int32_t* leaf, void* stream) {
  if (n < 0 || n >= gw::kMaxRows || F < 1 || F > INT32_MAX || T < 0 || T >= gw::kMaxRows || N < 0 || N >= gw::kMaxRows ||
      steps < 0 || steps > gw::kMaxSteps || (leaf && n * T >= gw::kMaxRows))
    return MP4X_E_BADARG;
  if (n == 0) return 0;
  if (!bins || !pred || ((uintptr_t)pred & 7) || ((uintptr_t)init & 7) || ((uintptr_t)leaf & 3) ||
      (T && (!tree_off || ((uintptr_t)tree_off & 3))) || (N && (!nodes || ((uintptr_t)nodes & 15) || !value || ((uintptr_t)value & 7))))
    return MP4X_E_BADARG;
  const gw::Shape sh = gw::shape(F);
  const dim3 grid((unsigned)((n + gw::kRowTile - 1) / gw::kRowTile));
  const size_t lds = (size_t)gw::kChunkBytes + (sh.lds ? (size_t)sh.stride * gw::kRowTile : 0);
  if (sh.lds)
    hipLaunchKernelGGL(k_gbdt_predict<true>, grid, dim3(kBlock), lds, (hipStream_t)stream, bins, (const int4*)nodes, value,
                       tree_off, init, n, F, T, (int32_t)N, steps, pred, leaf);
  else
    hipLaunchKernelGGL(k_gbdt_predict<false>, grid, dim3(kBlock), lds, (hipStream_t)stream, bins, (const int4*)nodes, value,
                       tree_off, init, n, F, T, (int32_t)N, steps, pred, leaf);
  return (int)hipGetLastError();
}
