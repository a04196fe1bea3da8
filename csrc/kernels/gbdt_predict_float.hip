// K20 — GBDT forest prediction from float features: a key-threshold LDS tree walk (gfx950).
//
//   pred[r] = init[r] (or +0.0) + sum over the trees t = 0 .. T-1, in that order, of value[o[t] + j(r, t)]
//   leaf[r, t] = j(r, t), the node the walk of row r in tree t ends on (-1 for a tree without nodes)
//
// K18's walk (gbdt_walk_map.hpp: tree table, chunk plan, is_inner) over rows of float32, float16 or bfloat16
// features: a node's threshold is a uint32 key K and the row moves right iff K <= xkey(x)
// (gbdt_fwalk_map.hpp).  No bin tensor: with the keys of float_forest the result is bin-then-walk's.
//
//   k_gbdt_predict_float<DT, U>   U >= 1: a block per tile of 256 * U consecutive rows (U = 4, 2, 1 by F); a
//                    thread owns U of them (tile + u * 256 + tid) and keeps their float64 sums in registers
//                    from the first chunk to the last, so the sum's order is the tree order.
//                    Keys: the tile's elements are one contiguous range of X; 16-byte loads over its aligned
//                    middle (4 or 8 elements) and element loads at the ragged head and tail; every element
//                    is widened, turned into its key (NaN: kNanKey) and stored once into LDS rows of F | 1
//                    dwords.  The float is not looked at again.
//                    Forest: K18's chunks.  A window of kChunkTrees raw offsets stands in LDS (two windows in
//                    turn), every thread runs next_chunk over it, then the chunk's node records and values
//                    are staged with coalesced loads.  Per tree the U walks of a lane are interleaved: a
//                    step of a row is one 16-byte LDS read of the node, one 4-byte LDS read of the key and
//                    an unsigned compare.  The step loop has exactly `steps` trips; a wave leaves it when a
//                    ballot says no lane stands on an inner node.  A tree larger than kChunkNodes is walked
//                    from global memory by the same code.  Two barriers a chunk.
//   k_gbdt_predict_float<DT, 0>   F >= kGlobalF: the keys of a tile do not fit; four rows a lane, every step
//                    reads its element of X from global memory and forms the key there.
//
// Integer compares and float64 additions (one a tree and row, in tree order) only: no float mode matters,
// nothing to contract.  No atomics, no scratch, no allocation and no host read: recordable in a graph.
#include "common.hpp"
#include "gbdt_fwalk_map.hpp"

namespace mp4x {

namespace gw = gbdt_walk;
namespace gf = gbdt_fwalk;
static_assert(gw::kBlock == kBlock, "a block is kBlock threads");

template <int DT> __device__ __forceinline__ uint32_t key_of(typename Elem<DT>::S s) {
  return gf::xkey(__float_as_uint(Elem<DT>::load(s)));
}

// The walks of a lane's R rows through one tree of `size` > 0 nodes at nd / val (LDS or global memory), and
// the tree's term of every sum.  LDS: row_at[u] is the row's dword offset in the tile of keys, else its
// element offset in X.
template <int DT, bool LDS, int R>
__device__ __forceinline__ void fwalk_tree(const int4* nd, const double* val, int32_t size, int64_t F, int steps,
                                           const uint32_t* keys, const typename Elem<DT>::S* __restrict__ X,
                                           const int64_t (&row_at)[R], int32_t (&j)[R], double (&acc)[R]) {
#pragma unroll
  for (int u = 0; u < R; ++u) j[u] = 0;
  for (int s = 0; s < steps; ++s) {
    gw::Node rec[R];
    uint32_t xk[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      MP4X_DASSERT(j[u] >= 0 && j[u] < size);
      const int4 v = nd[j[u]];
      rec[u] = gw::Node{v.x, v.y, v.z, v.w};
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int64_t f = gw::bin_feature(rec[u], size, F);
      xk[u] = LDS ? keys[row_at[u] + f] : key_of<DT>(X[row_at[u] + f]);
    }
    bool moved = false;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int32_t nx = gf::step(rec[u], size, F, xk[u]);
      moved |= nx >= 0;
      j[u] = nx >= 0 ? nx : j[u];
    }
    if (!__any(moved)) break;                            // wave-uniform: every lane stands on a non-inner node
  }
#pragma unroll
  for (int u = 0; u < R; ++u) acc[u] += val[j[u]];
}

template <int DT, int U>
__global__ __launch_bounds__(kBlock) void k_gbdt_predict_float(const typename Elem<DT>::S* __restrict__ X,
                                                               const int4* __restrict__ nodes,
                                                               const double* __restrict__ value,
                                                               const int32_t* __restrict__ tree_off, const double* init,
                                                               int64_t n, int64_t F, int64_t T, int32_t N, int steps,
                                                               double* pred, int32_t* __restrict__ leaf) {
  using S = typename Elem<DT>::S;
  constexpr bool LDS = U > 0;
  constexpr int R = LDS ? U : gf::kGlobalRows, kTile = kBlock * R, kVec = 16 / (int)sizeof(S);
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  int4* const s_nodes = (int4*)lds;
  double* const s_val = (double*)(lds + gw::kChunkNodes * 16);
  int32_t* const s_win = (int32_t*)(lds + gw::kChunkNodes * 24);      // [2][kChunkTrees]
  uint32_t* const s_keys = (uint32_t*)(lds + gw::kChunkBytes);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kTile;
  const int64_t rows = gf::tile_rows(n, blockIdx.x, kTile);          // >= 1: the grid is ceil(n / kTile)
  const int stride = (int)gf::stride_dw(F);

  if (LDS) {                                             // the tile's elements: one contiguous range of X
    const S* src = X + row0 * F;
    const int Fi = (int)F, elems = (int)rows * Fi;       // F < kGlobalF: a tile's elements fit an int
    const gw::Span sp = gw::span16((uint64_t)(uintptr_t)src, (uint64_t)(uintptr_t)(src + elems));
    // X is aligned to its element, so both ends of the aligned middle are whole elements
    const int head = (int)((sp.head_end - (uint64_t)(uintptr_t)src) / sizeof(S));
    const int tail = (int)((sp.tail_begin - (uint64_t)(uintptr_t)src) / sizeof(S));
    for (int i = tid; i < head; i += kBlock) s_keys[(i / Fi) * stride + i % Fi] = key_of<DT>(src[i]);
    for (int i = tail + tid; i < elems; i += kBlock) s_keys[(i / Fi) * stride + i % Fi] = key_of<DT>(src[i]);
    for (int i = head + tid * kVec; i < tail; i += kBlock * kVec) {
      const u32x4 v = *(const u32x4*)(src + i);
      int r = i / Fi, c = i - r * Fi;
#pragma unroll
      for (int b = 0; b < kVec; ++b) {
        const uint32_t w = v[b * (int)sizeof(S) / 4];
        S e;
        if constexpr (sizeof(S) == 4) e = __uint_as_float(w);
        else e = (S)(w >> ((b & 1) * 16));
        s_keys[r * stride + c] = key_of<DT>(e);
        if (++c == Fi) {
          c = 0;
          ++r;
        }
      }
    }
  }

  int64_t row_at[R];
  bool live[R];
  double acc[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int lr = gw::lane_row(tid, u);
    live[u] = lr < rows;
    const int64_t r = live[u] ? lr : rows - 1;           // a lane past the end walks the last row, stores nothing
    row_at[u] = LDS ? r * stride : (row0 + r) * F;
    acc[u] = live[u] && init ? init[row0 + lr] : 0.0;
  }

  if (T > 0 && tid < gw::window(T, 0)) s_win[tid] = tree_off[1 + tid];
  __syncthreads();                                       // the keys and the first window stand
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
      int32_t j[R];
      if (size > 0) {
        if (c.big) fwalk_tree<DT, LDS, R>(nodes + lo, value + lo, size, F, steps, s_keys, X, row_at, j, acc);
        else fwalk_tree<DT, LDS, R>(s_nodes + (lo - o0), s_val + (lo - o0), size, F, steps, s_keys, X, row_at, j, acc);
      }
      if (leaf) {
#pragma unroll
        for (int u = 0; u < R; ++u)
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
  for (int u = 0; u < R; ++u)
    if (live[u]) pred[row0 + gw::lane_row(tid, u)] = acc[u];
}

}  // namespace mp4x

using namespace mp4x;

extern "C" int mp4x_gbdt_predict_float(const void* X, int dtype, const int32_t* nodes, const double* value,
                                       const int32_t* tree_off, const double* init, int64_t n, int64_t F, int64_t T,
                                       int64_t N, int steps, double* pred, int32_t* leaf, void* stream) {
  if (n < 0 || n >= gw::kMaxRows || F < 1 || F > INT32_MAX || T < 0 || T >= gw::kMaxRows || N < 0 || N >= gw::kMaxRows ||
      steps < 0 || steps > gw::kMaxSteps || (leaf && n * T >= gw::kMaxRows) ||
      (dtype != MP4X_F32 && dtype != MP4X_F16 && dtype != MP4X_BF16))
    return MP4X_E_BADARG;
  if (n == 0) return 0;
  if (!X || ((uintptr_t)X & (dtype == MP4X_F32 ? 3 : 1)) || !pred || ((uintptr_t)pred & 7) || ((uintptr_t)init & 7) ||
      ((uintptr_t)leaf & 3) || (T && (!tree_off || ((uintptr_t)tree_off & 3))) ||
      (N && (!nodes || ((uintptr_t)nodes & 15) || !value || ((uintptr_t)value & 7))))
    return MP4X_E_BADARG;
  const int tile = gf::tile_rows_of(F);
  const dim3 grid((unsigned)((n + tile - 1) / tile));
  const size_t lds = (size_t)gf::lds_bytes(F);
  auto launch = [&](auto dtc, auto uc) {
    constexpr int DT = decltype(dtc)::value, U = decltype(uc)::value;
    hipLaunchKernelGGL((k_gbdt_predict_float<DT, U>), grid, dim3(kBlock), lds, (hipStream_t)stream,
                       (const typename Elem<DT>::S*)X, (const int4*)nodes, value, tree_off, init, n, F, T, (int32_t)N, steps,
                       pred, leaf);
    return (int)hipGetLastError();
  };
  auto by_rows = [&](auto dtc) {
    switch (gf::rows_per_lane(F)) {
      case 4: return launch(dtc, IntC<4>{});
      case 2: return launch(dtc, IntC<2>{});
      case 1: return launch(dtc, IntC<1>{});
      default: return launch(dtc, IntC<0>{});
    }
  };
  if (dtype == MP4X_F32) return by_rows(IntC<MP4X_F32>{});
  if (dtype == MP4X_F16) return by_rows(IntC<MP4X_F16>{});
  return by_rows(IntC<MP4X_BF16>{});
}
