// K9 — expert-parallel token routing on the GPU (gfx950): the kernels around the ragged
// all-to-all of a mixture-of-experts layer.
//
// Assignments are flattened token-major: a = t * K + k, n = T * K; the bucket of an assignment
// is its expert id itself (0 <= id < nb, nb <= 2048).  A negative id and an id >= nb are placed
// nowhere; they are counted in two buckets of their own behind the experts, so the same scan
// serves them and they never move an expert's base.
//
//   route count    k_moe_hist     per-256-assignment tile LDS histogram -> hist[b * nblk + tile]
//                  DeviceScan     exclusive sum over (bucket-major, tile-minor)
//                  k_moe_counts   counts[nb + 2] from the scanned bases
//   route scatter  k_moe_scatter  K4b's ballot ranks (csrc/kernels/sparse.hip k_pack_scatter):
//                  slots[a] = base(bucket, tile) + rank inside the tile, staged in LDS, then lane
//                  groups replicate token rows (16-B loads) into their slots (nontemporal stores),
//                  optionally scaled per assignment (one multiply per element, one rounding);
//                  up to 16 blocks share a tile of long rows (tile_split); with an expert
//                  capacity (CLIP) an assignment past its expert's quota gets slot -1 there and
//                  its row is neither read nor written; with a per-source share (PAD) the
//                  pe-th assignment of expert e goes to the fixed slot e * cap + pe iff pe < cap
//   pad fill       k_moe_pad_fill  zeros to the rows [min(cnt[e], cap), cap) of every expert block
//                  of the padded layout, so every row of the buffer is written exactly once
//   pad counts     k_moe_pad_counts  kept[e] = min(cnt[e], cap) and dropped[3] (over the share,
//                  negative, >= nb) from the scanned bases
//   combine        k_moe_combine  out[t] = sum over k, in k order, of w[t, k] * rows[slots[t, k]]:
//                  a lane group per token reads its K rows through the slot index; the mul and
//                  the add are separate roundings (no contraction), one rounding to the dtype
//   combine bwd    k_moe_combine_bwd  (K11) both gradients of the combine from one pass over its output
//                  gradient g: g_rows[slots[t, k]] = w[t, k] * g[t] (the scatter's bits with row_scale)
//                  and g_w[t, k] = g[t] . rows[slots[t, k]] in f32, the same lane groups, no temporary
//
// The slot order is exactly the stable sort by expert id.  No global atomics anywhere: every
// result is identical run to run.
#include <rocprim/device/device_scan.hpp>

#include "common.hpp"

namespace mp4x {

constexpr int kMoeMaxNb = 2048;      // K4b's kPackMaxP: 4 * nb * 4 B + 2 KiB of LDS in the scatter

__device__ __forceinline__ int64_t moe_id(const void* __restrict__ ids, int is_i64, int64_t i) {
  return is_i64 ? reinterpret_cast<const int64_t*>(ids)[i] : (int64_t)reinterpret_cast<const int32_t*>(ids)[i];
}

// acc + w * x with the product and the sum rounded separately, as the eager CPU reference does.
// hipcc contracts device code by default (and __fmul_rn / __fadd_rn are a plain * and + to it), so
// contraction is switched off here, where the pragma is honoured.
__device__ __forceinline__ float mul_rn(float w, float x) {
#pragma clang fp contract(off)
  return w * x;
}
__device__ __forceinline__ float mul_add_rn(float acc, float w, float x) {
#pragma clang fp contract(off)
  const float prod = w * x;
  return acc + prod;
}

// Histogram bucket: the expert, or nb (negative: dropped by the caller) / nb + 1 (out of range).
__device__ __forceinline__ int moe_bucket(int64_t id, int nb) { return id < 0 ? nb : (id >= nb ? nb + 1 : (int)id); }

__global__ __launch_bounds__(kBlock) void k_moe_hist(const void* __restrict__ ids, int is_i64, int64_t n, int nb,
                                                     int64_t nblk, int64_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) int32_t lh[];
  const int nbk = nb + 2;
  for (int i = threadIdx.x; i < nbk; i += kBlock) lh[i] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) atomicAdd(&lh[moe_bucket(moe_id(ids, is_i64, i), nb)], 1);
  __syncthreads();
  for (int d = threadIdx.x; d < nbk; d += kBlock) hist[(int64_t)d * nblk + blockIdx.x] = lh[d];
}

// One block: counts[q] = assignments of bucket q from the scanned (bucket, tile) bases.
__global__ __launch_bounds__(kBlock) void k_moe_counts(const int64_t* __restrict__ off, const int64_t* __restrict__ hist,
                                                       int nbk, int64_t nblk, int64_t* __restrict__ counts) {
  const int64_t last = (int64_t)nbk * nblk - 1;
  for (int q = threadIdx.x; q < nbk; q += kBlock) {
    const int64_t end = (q + 1 < nbk) ? off[(int64_t)(q + 1) * nblk] : off[last] + hist[last];
    counts[q] = end - off[(int64_t)q * nblk];
  }
}

// CLIP (an expert capacity): clip[0 .. nb) = keep[e], the rows of expert e this rank may send, and
// clip[nb .. 2 nb) = kept_base[e], the exclusive prefix of keep.  The position of an assignment
// inside its expert is its unclipped slot less the expert's unclipped base off[e * nblk]; it stays
// iff that is below keep[e], at kept_base[e] + position.  Three gathers per placed lane from tables
// of at most 2048 entries (L2 hits; not staged in LDS, which would cost occupancy).
//
// PAD (a per-source share, the padded fixed-capacity layout): every expert owns the block of `cap`
// rows [e * cap, (e + 1) * cap) whatever the ids are; the position stays iff it is below cap, at
// e * cap + position.  cap is a scalar: no table at all.  The rows of a block no assignment reaches
// are k_moe_pad_fill's.
enum : int { kMoePlain = 0, kMoeClip = 1, kMoePad = 2 };

template <int DT, bool SCALED, int MODE>
__global__ __launch_bounds__(kBlock) void k_moe_scatter(const void* __restrict__ ids, int is_i64,
                                                        const u32x4* __restrict__ x,
                                                        const float* __restrict__ row_scale, int64_t n, int K,
                                                        int64_t V, int G, int nb, int64_t nblk, int S,
                                                        const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ clip, int64_t cap,
                                                        u32x4* __restrict__ out_rows, int64_t* __restrict__ slots) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* wcnt = reinterpret_cast<int32_t*>(smem);                            // [4][nb]
  int64_t* pos = reinterpret_cast<int64_t*>(smem + ((4 * nb * 4 + 15) & ~15));   // [kBlock]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  // S blocks share a tile: each ranks the tile's 256 ids again (cheap) and moves every S-th
  // group of its rows, so few tiles of long rows still fill the device
  const int64_t b = blockIdx.x / S, t0 = b * kBlock, i = t0 + tid;
  const int part = blockIdx.x % S;
  for (int j = tid; j < 4 * nb; j += kBlock) wcnt[j] = 0;
  __syncthreads();
  const int64_t id = i < n ? moe_id(ids, is_i64, i) : -1;
  const bool placed = id >= 0 && id < nb;
  const int d = placed ? (int)id : -1;
  uint64_t active = __ballot(placed);
  int rank = 0;
  while (active) {                       // wave-uniform: one trip per distinct expert in the wave
    const int leader = __ffsll((unsigned long long)active) - 1;
    const int ld = __shfl(d, leader);
    const uint64_t m = __ballot(d == ld) & active;
    if (d == ld) rank = __popcll(m & ((1ull << lane) - 1));
    if (lane == leader) wcnt[w * nb + ld] = __popcll(m);
    active &= ~m;
  }
  __syncthreads();
  int64_t ps = -1;
  if (placed) {
    int inb = rank;
    for (int q = 0; q < w; ++q) inb += wcnt[q * nb + d];
    ps = off[(int64_t)d * nblk + b] + inb;
    MP4X_DASSERT(ps >= 0 && ps < n);
    if constexpr (MODE == kMoeClip) {
      const int64_t pe = ps - off[(int64_t)d * nblk];
      ps = pe < clip[d] ? clip[nb + d] + pe : -1;
      MP4X_DASSERT(ps < clip[nb - 1] + clip[2 * nb - 1]);          // the kept total
    }
    if constexpr (MODE == kMoePad) {
      const int64_t pe = ps - off[(int64_t)d * nblk];
      ps = pe < cap ? (int64_t)d * cap + pe : -1;
      MP4X_DASSERT(ps < (int64_t)nb * cap);
    }
  }
  if (i < n && part == 0) slots[i] = ps;
  pos[tid] = ps;
  __syncthreads();
  const int64_t rows = (n - t0) < kBlock ? (n - t0) : kBlock;
  const int grp = lane / G, sub = lane % G, R = 64 / G;
  constexpr int UNR = 4;
  int it = 0;
  for (int r0 = w * R + grp; r0 < rows; r0 += 4 * R * UNR, ++it) {
    if (it % S != part) continue;
    for (int64_t v = sub; v < V; v += G) {
      u32x4 y[UNR];
      int64_t dst[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int r = r0 + u * 4 * R;
        dst[u] = r < rows ? pos[r] : -1;
        // the K assignments of a token sit next to each other in the tile: its row is read from
        // memory once and from the cache K - 1 times, so the loads stay temporal
        // (n <= INT32_MAX / 2: the token index is a 32-bit division)
        if (dst[u] >= 0) y[u] = x[(int64_t)((uint32_t)(t0 + r) / (uint32_t)K) * V + v];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (dst[u] < 0) continue;
        if constexpr (SCALED) {
          constexpr int W = 16 / sizeof(typename Elem<DT>::S);
          const float s = row_scale[t0 + r0 + u * 4 * R];
          float a[W];
          unpack<DT>(y[u], a);
#pragma unroll
          for (int j = 0; j < W; ++j) a[j] = mul_rn(s, a[j]);
          y[u] = pack<DT, u32x4>(a);
        }
        __builtin_nontemporal_store(y[u], out_rows + dst[u] * V + v);
      }
    }
  }
}

// The pad rows of the padded layout.  The rows [min(cnt[e], cap), cap) of expert e's block are one
// contiguous span of (cap - kept) * V vectors, so the lanes of a block walk it vector by vector
// (consecutive lanes, consecutive 16-byte nontemporal stores: whole 1 KiB lines per wave, which a
// lane group per row would only reach for V >= 64); blockIdx.y is the expert, blockIdx.x strides
// over the span.  cnt[e] comes from the scanned bases; off == nullptr is the call with no
// assignment at all (nothing was scanned): every row is pad.
__global__ __launch_bounds__(kBlock) void k_moe_pad_fill(const int64_t* __restrict__ off, int64_t nblk, int64_t cap,
                                                         int64_t V, u32x4* __restrict__ out_rows) {
  const int e = blockIdx.y;
  int64_t kept = 0;
  if (off) {
    kept = off[(int64_t)(e + 1) * nblk] - off[(int64_t)e * nblk];       // bucket e + 1 exists: nb + 2 buckets
    if (kept > cap) kept = cap;
  }
  const int64_t span = (cap - kept) * V;
  u32x4* dst = out_rows + ((int64_t)e * cap + kept) * V;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < span; v += (int64_t)gridDim.x * kBlock)
    __builtin_nontemporal_store(zero, dst + v);
}

// One block: kept[e] = min(cnt[e], cap), written at wire[(e / el) * el_pad + e % el] (el_pad >= el:
// every destination rank's counts start on a 16-byte boundary of the exchange; el_pad == el is the
// plain [nb] vector), and dropped = {over the share, negative ids, ids >= nb}.  Integer sums only:
// identical run to run.  off == nullptr: no assignment at all.
__global__ __launch_bounds__(kBlock) void k_moe_pad_counts(const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ hist, int nb, int64_t nblk,
                                                           int64_t cap, int el, int el_pad, int64_t* __restrict__ wire,
                                                           int64_t* __restrict__ dropped) {
  __shared__ unsigned long long over;
  if (threadIdx.x == 0) over = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (int e = threadIdx.x; e < nb; e += kBlock) {
    const int64_t c = off ? off[(int64_t)(e + 1) * nblk] - off[(int64_t)e * nblk] : 0;
    const int64_t k = c < cap ? c : cap;
    wire[(int64_t)(e / el) * el_pad + e % el] = k;
    mine += (unsigned long long)(c - k);
  }
  for (int q = threadIdx.x; q < (nb / el) * (el_pad - el); q += kBlock)      // the wire's padding
    wire[(int64_t)(q / (el_pad - el)) * el_pad + el + q % (el_pad - el)] = 0;
  if (mine) atomicAdd(&over, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t last = (int64_t)(nb + 2) * nblk - 1;
    dropped[0] = (int64_t)over;
    dropped[1] = off ? off[(int64_t)(nb + 1) * nblk] - off[(int64_t)nb * nblk] : 0;
    dropped[2] = off ? off[last] + hist[last] - off[(int64_t)(nb + 1) * nblk] : 0;
  }
}

// G lanes per token (64 / G tokens per wave); a lane owns the 16-byte vectors sub, sub + G, ... of
// the row and walks the token's K slots in k order.  nrows bounds a slot (debug builds): T * K in
// the ragged layout, nb * cap in the padded one.
template <int DT>
__global__ __launch_bounds__(kBlock) void k_moe_combine(const u32x4* __restrict__ rows,
                                                        const int64_t* __restrict__ slots,
                                                        const float* __restrict__ weights, int64_t T, int K,
                                                        int64_t V, int G, int64_t nrows,
                                                        u32x4* __restrict__ out) {
  constexpr int W = 16 / sizeof(typename Elem<DT>::S);
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, sub = lane % G, R = 64 / G;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
  for (int64_t t = wave * R + grp; t < T; t += nwaves * R) {
    const int64_t* sl = slots + t * K;
    const float* wt = weights ? weights + t * K : nullptr;
    for (int64_t v = sub; v < V; v += G) {
      float acc[W];
#pragma unroll
      for (int j = 0; j < W; ++j) acc[j] = 0.0f;
      for (int k = 0; k < K; ++k) {
        const int64_t s = sl[k];
        if (s < 0) continue;
        MP4X_DASSERT(s < nrows);
        const float wk = wt ? wt[k] : 1.0f;
        float a[W];
        unpack<DT>(rows[s * V + v], a);
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = mul_add_rn(acc[j], wk, a[j]);
      }
      out[t * V + v] = pack<DT, u32x4>(acc);
    }
  }
}

// K11, the combine's backward in one pass over g: the lane groups of k_moe_combine.  A lane owns
// the vectors sub, sub + G, ... of g[t]; per vector it loads g once, issues the loads of the (at
// most kMoeBwdMaxK) live rows[slot] together, folds each into its slot's partial dot product (f32,
// contraction allowed) and stores w * g (mul_rn: one multiply, one rounding) to g_rows[slot],
// nontemporal.  The k loop has the fixed trip count kMoeBwdMaxK under the uniform guard k < K, so
// slots, weights and partial sums sit in registers under compile-time indices (no scratch).  After
// the row a __shfl_xor tree per k over the group, and lane 0 of the group writes g_weights: the
// summation order is a function of (dtype, width) alone.  A slot < 0 reads and writes no row and
// gives +0.0f.  No LDS, no atomics.  KMAX (4, 8 or 16, the smallest that holds K) only sizes those
// registers: a small K keeps more waves resident; the arithmetic and its order do not depend on it.
constexpr int kMoeBwdMaxK = 16;

template <int DT, int KMAX>
__global__ __launch_bounds__(kBlock) void k_moe_combine_bwd(const u32x4* __restrict__ g,
                                                            const u32x4* __restrict__ rows,
                                                            const int64_t* __restrict__ slots,
                                                            const float* __restrict__ weights, int64_t T, int K,
                                                            int64_t V, int G, int64_t nrows,
                                                            u32x4* __restrict__ g_rows,
                                                            float* __restrict__ g_weights) {
  constexpr int W = 16 / sizeof(typename Elem<DT>::S);
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, sub = lane % G, R = 64 / G;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
  for (int64_t t = wave * R + grp; t < T; t += nwaves * R) {
    const int64_t* sl = slots + t * K;
    const float* wt = weights + t * K;
    int64_t base[KMAX];            // slot * V, or -1
    float wk[KMAX], dot[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      base[k] = -1;
      wk[k] = 0.0f;
      dot[k] = 0.0f;
      if (k < K) {
        const int64_t s = sl[k];
        MP4X_DASSERT(s < nrows);
        base[k] = s < 0 ? -1 : s * V;
        wk[k] = wt[k];
      }
    }
    for (int64_t v = sub; v < V; v += G) {
      float a[W];
      unpack<DT>(g[t * V + v], a);
      u32x4 y[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K && base[k] >= 0) y[k] = rows[base[k] + v];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K && base[k] >= 0) {
          float b[W];
          unpack<DT>(y[k], b);
#pragma unroll
          for (int j = 0; j < W; ++j) dot[k] = __builtin_fmaf(a[j], b[j], dot[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K && base[k] >= 0) {
          float b[W];
#pragma unroll
          for (int j = 0; j < W; ++j) b[j] = mul_rn(wk[k], a[j]);
          __builtin_nontemporal_store(pack<DT, u32x4>(b), g_rows + base[k] + v);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        float d = dot[k];
        for (int m = G >> 1; m > 0; m >>= 1) d += __shfl_xor(d, m);
        if (sub == 0) g_weights[t * K + k] = d;
      }
    }
  }
}

}  // namespace mp4x

using namespace mp4x;

namespace {
size_t moe_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct MoeScratch {
  int64_t nblk, m;
  int64_t *hist, *off;
  void* temp;
  size_t temp_bytes;
};

MoeScratch moe_scratch(void* scratch, size_t scratch_bytes, int64_t n, int nb) {
  MoeScratch S;
  S.nblk = (n + kBlock - 1) / kBlock;
  S.m = (int64_t)(nb + 2) * S.nblk;
  char* sc = (char*)scratch;
  const size_t head = 2 * moe_align(S.m * sizeof(int64_t));
  S.hist = (int64_t*)sc;
  S.off = (int64_t*)(sc + head / 2);
  S.temp = sc + head;
  S.temp_bytes = scratch_bytes - head;
  return S;
}

// f32 / bf16 / f16 are the routed dtypes: 0, else MP4X_E_UNSUPPORTED.
int moe_dtype_ok(int dtype) { return (dtype == MP4X_F32 || dtype == MP4X_BF16 || dtype == MP4X_F16) ? 0 : MP4X_E_UNSUPPORTED; }

int lane_group(int64_t V) {
  int G = 1;
  while (G < V && G < 64) G <<= 1;
  return G;
}

// Blocks per tile of the scatter: towards 4 blocks per CU (1024) when the tiles alone are fewer,
// while every block still moves at least 2048 vectors (32 KiB); never more than the 256 / (16 *
// 64 / G) row groups of a tile (V / 8 <= G / 4 for every V), at most 16.
int tile_split(int64_t nblk, int64_t V) {
  int64_t s = 1024 / nblk;
  if (s > V / 8) s = V / 8;
  return (int)(s < 1 ? 1 : (s > 16 ? 16 : s));
}
}  // namespace

extern "C" size_t mp4x_moe_route_scratch_bytes(int64_t n, int nb) {
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  const int64_t m = (int64_t)(nb + 2) * (nblk < 1 ? 1 : nblk);
  size_t cub_bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, cub_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)m,
                                rocprim::plus<int64_t>(), (hipStream_t)0);
  return 2 * moe_align(m * sizeof(int64_t)) + moe_align(cub_bytes);
}

extern "C" int mp4x_moe_route_count(const void* ids, int ids_are_i64, int64_t n, int nb, int64_t* counts,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (nb < 1 || nb > kMoeMaxNb || n < 0 || !counts || ((uintptr_t)counts & 7)) return MP4X_E_BADARG;
  if (n == 0) return (int)hipMemsetAsync(counts, 0, (nb + 2) * sizeof(int64_t), st);
  if (n > INT32_MAX / 2 || !ids || ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) || !scratch || ((uintptr_t)scratch & 255))
    return MP4X_E_BADARG;
  if (scratch_bytes < mp4x_moe_route_scratch_bytes(n, nb)) return MP4X_E_BADARG;
  MoeScratch S = moe_scratch(scratch, scratch_bytes, n, nb);
  hipLaunchKernelGGL(k_moe_hist, dim3(S.nblk), dim3(kBlock), (nb + 2) * sizeof(int32_t), st, ids, ids_are_i64, n, nb,
                     S.nblk, S.hist);
  int e = (int)hipGetLastError();
  if (e) return e;
  e = (int)rocprim::exclusive_scan(S.temp, S.temp_bytes, S.hist, S.off, (int64_t)0, (size_t)S.m,
                                   rocprim::plus<int64_t>(), st);
  if (e) return e;
  hipLaunchKernelGGL(k_moe_counts, dim3(1), dim3(kBlock), 0, st, (const int64_t*)S.off, (const int64_t*)S.hist, nb + 2,
                     S.nblk, counts);
  return (int)hipGetLastError();
}

namespace {
// The pad rows of every expert block; sc == nullptr: no assignment, the whole buffer is pad.
int moe_pad_fill_launch(const MoeScratch* sc, int nb, int64_t cap, int64_t V, void* out_rows, hipStream_t st) {
  const int64_t span = cap * V;
  int64_t gx = (span + 4 * kBlock - 1) / (4 * kBlock);           // >= 4 vectors (64 B) per lane of a full block
  const int64_t room = 4096 / nb;                                // ... and about 16 blocks per CU in all
  if (gx > room) gx = room;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(k_moe_pad_fill, dim3((unsigned)gx, (unsigned)nb), dim3(kBlock), 0, st,
                     sc ? (const int64_t*)sc->off : (const int64_t*)nullptr, sc ? sc->nblk : 0, cap, V, (u32x4*)out_rows);
  return (int)hipGetLastError();
}

// The scatter entry points: kMoePlain has no table, kMoeClip reads clip, kMoePad the scalar cap.
template <int MODE>
int moe_scatter_launch(int dtype, const void* ids, int ids_are_i64, const void* x, const float* row_scale, int64_t n,
                       int K, int64_t row_bytes, int nb, void* out_rows, int64_t* slots, const int64_t* clip,
                       int64_t cap, void* scratch, size_t scratch_bytes, void* stream) {
  constexpr bool PAD = MODE == kMoePad;
  if (int e = moe_dtype_ok(dtype)) return e;
  if (nb < 1 || nb > kMoeMaxNb || n < 0 || K < 1 || n % K || row_bytes < 16 || (row_bytes & 15)) return MP4X_E_BADARG;
  if (MODE == kMoeClip && (!clip || ((uintptr_t)clip & 7))) return MP4X_E_BADARG;
  // the padded buffer is written whole even without an assignment: it is checked before the empty call
  if (PAD && (cap < 1 || cap > INT32_MAX / nb || !out_rows || ((uintptr_t)out_rows & 15))) return MP4X_E_BADARG;
  if (n == 0) return PAD ? moe_pad_fill_launch(nullptr, nb, cap, row_bytes / 16, out_rows, (hipStream_t)stream) : 0;
  if (n > INT32_MAX / 2 || !ids || ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) || !x || !out_rows ||
      (((uintptr_t)x | (uintptr_t)out_rows) & 15) || !slots || ((uintptr_t)slots & 7) || ((uintptr_t)row_scale & 3) ||
      !scratch || ((uintptr_t)scratch & 255))
    return MP4X_E_BADARG;
  if (scratch_bytes < mp4x_moe_route_scratch_bytes(n, nb)) return MP4X_E_BADARG;
  const MoeScratch S_ = moe_scratch(scratch, scratch_bytes, n, nb);
  const int64_t V = row_bytes / 16;
  const int G = lane_group(V);
  const size_t lds = ((4 * nb * 4 + 15) & ~15) + kBlock * sizeof(int64_t);
  const int S = tile_split(S_.nblk, V);
  hipStream_t st = (hipStream_t)stream;
  if (!row_scale) {                      // whole rows move as bytes: one instantiation serves every dtype
    hipLaunchKernelGGL((k_moe_scatter<MP4X_F32, false, MODE>), dim3(S_.nblk * S), dim3(kBlock), lds, st, ids,
                       ids_are_i64, (const u32x4*)x, row_scale, n, K, V, G, nb, S_.nblk, S, (const int64_t*)S_.off, clip, cap,
                       (u32x4*)out_rows, slots);
    if (int e = (int)hipGetLastError()) return e;
    return PAD ? moe_pad_fill_launch(&S_, nb, cap, V, out_rows, st) : 0;
  }
  const int e = with_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    if constexpr (DT == MP4X_F32 || DT == MP4X_BF16 || DT == MP4X_F16) {
      hipLaunchKernelGGL((k_moe_scatter<DT, true, MODE>), dim3(S_.nblk * S), dim3(kBlock), lds, st, ids, ids_are_i64,
                         (const u32x4*)x, row_scale, n, K, V, G, nb, S_.nblk, S, (const int64_t*)S_.off, clip, cap,
                         (u32x4*)out_rows, slots);
      return (int)hipGetLastError();
    } else {
      return (int)MP4X_E_UNSUPPORTED;
    }
  });
  if (e) return e;
  return PAD ? moe_pad_fill_launch(&S_, nb, cap, V, out_rows, st) : 0;
}
}  // namespace

extern "C" int mp4x_moe_route_scatter(int dtype, const void* ids, int ids_are_i64, const void* x,
                                      const float* row_scale, int64_t n, int K, int64_t row_bytes, int nb,
                                      void* out_rows, int64_t* slots, void* scratch, size_t scratch_bytes,
                                      void* stream) {
  return moe_scatter_launch<kMoePlain>(dtype, ids, ids_are_i64, x, row_scale, n, K, row_bytes, nb, out_rows, slots,
                                       nullptr, 0, scratch, scratch_bytes, stream);
}

extern "C" int mp4x_moe_route_scatter_clip(int dtype, const void* ids, int ids_are_i64, const void* x,
                                           const float* row_scale, int64_t n, int K, int64_t row_bytes, int nb,
                                           void* out_rows, int64_t* slots, const int64_t* clip, void* scratch,
                                           size_t scratch_bytes, void* stream) {
  return moe_scatter_launch<kMoeClip>(dtype, ids, ids_are_i64, x, row_scale, n, K, row_bytes, nb, out_rows, slots, clip,
                                      0, scratch, scratch_bytes, stream);
}

// The padded fixed-capacity layout: out_rows holds nb * cap rows and every one of them is written
// exactly once, the kept rows by the scatter and the pad rows [min(cnt[e], cap), cap) of every
// expert block by the fill (a kernel of its own: it also serves the call with no assignment, where
// the scatter has no tile to launch, and its grid follows the expert blocks, not the tiles).
extern "C" int mp4x_moe_route_scatter_pad(int dtype, const void* ids, int ids_are_i64, const void* x,
                                          const float* row_scale, int64_t n, int K, int64_t row_bytes, int nb,
                                          int64_t cap, void* out_rows, int64_t* slots, void* scratch,
                                          size_t scratch_bytes, void* stream) {
  return moe_scatter_launch<kMoePad>(dtype, ids, ids_are_i64, x, row_scale, n, K, row_bytes, nb, out_rows, slots,
                                     nullptr, cap, scratch, scratch_bytes, stream);
}

// kept (min(cnt[e], cap), laid out [nb / el][el_pad]) and dropped[3] after mp4x_moe_route_count on
// the same scratch; n == 0 needs no scratch.
extern "C" int mp4x_moe_pad_counts(int64_t n, int nb, int64_t cap, int el, int el_pad, int64_t* kept, int64_t* dropped,
                                   void* scratch, size_t scratch_bytes, void* stream) {
  if (nb < 1 || nb > kMoeMaxNb || n < 0 || n > INT32_MAX / 2 || cap < 1 || el < 1 || nb % el || el_pad < el || !kept ||
      ((uintptr_t)kept & 7) || !dropped || ((uintptr_t)dropped & 7))
    return MP4X_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipLaunchKernelGGL(k_moe_pad_counts, dim3(1), dim3(kBlock), 0, st, (const int64_t*)nullptr, (const int64_t*)nullptr,
                       nb, (int64_t)0, cap, el, el_pad, kept, dropped);
    return (int)hipGetLastError();
  }
  if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < mp4x_moe_route_scratch_bytes(n, nb)) return MP4X_E_BADARG;
  const MoeScratch S = moe_scratch(scratch, scratch_bytes, n, nb);
  hipLaunchKernelGGL(k_moe_pad_counts, dim3(1), dim3(kBlock), 0, st, (const int64_t*)S.off, (const int64_t*)S.hist, nb,
                     S.nblk, cap, el, el_pad, kept, dropped);
  return (int)hipGetLastError();
}

namespace {
// Both combine entry points: num_rows < 0 is the ragged layout's bound T * K.
int moe_combine_launch(int dtype, const void* rows, int64_t num_rows, const int64_t* slots, const float* weights,
                       int64_t T, int K, int64_t width, void* out, void* stream) {
  if (int e = moe_dtype_ok(dtype)) return e;
  const int64_t row_bytes = width * elem_size(dtype);
  if (T < 0 || K < 1 || width < 1 || (row_bytes & 15)) return MP4X_E_BADARG;
  if (T == 0) return 0;
  // rows may be NULL only when nothing was placed, which the kernel cannot know: the caller passes
  // a valid (possibly one-row) buffer
  if (T > INT32_MAX / 2 / K || !rows || !out || (((uintptr_t)rows | (uintptr_t)out) & 15) || !slots ||
      ((uintptr_t)slots & 7) || ((uintptr_t)weights & 3))
    return MP4X_E_BADARG;
  const int64_t V = row_bytes / 16;
  const int G = lane_group(V);
  const int g = grid_for((T * G + 63) / 64 * 64, 1);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    if constexpr (DT == MP4X_F32 || DT == MP4X_BF16 || DT == MP4X_F16) {
      hipLaunchKernelGGL((k_moe_combine<DT>), dim3(g), dim3(kBlock), 0, st, (const u32x4*)rows, slots, weights, T, K, V,
                         G, num_rows < 0 ? T * K : num_rows, (u32x4*)out);
      return (int)hipGetLastError();
    } else {
      return (int)MP4X_E_UNSUPPORTED;
    }
  });
}
}  // namespace

extern "C" int mp4x_moe_combine(int dtype, const void* rows, const int64_t* slots, const float* weights, int64_t T,
                                int K, int64_t width, void* out, void* stream) {
  return moe_combine_launch(dtype, rows, -1, slots, weights, T, K, width, out, stream);
}

// The combine of the padded layout: slots reach num_rows - 1 = nb * cap - 1, which may exceed T * K.
extern "C" int mp4x_moe_combine_rows(int dtype, const void* rows, int64_t num_rows, const int64_t* slots,
                                     const float* weights, int64_t T, int K, int64_t width, void* out, void* stream) {
  if (num_rows < 1) return MP4X_E_BADARG;
  return moe_combine_launch(dtype, rows, num_rows, slots, weights, T, K, width, out, stream);
}

namespace {
bool moe_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)b_bytes && pb < pa + (uintptr_t)a_bytes;
}

// Both K11 entry points: everything they refuse, then the launch (none when T == 0).
int moe_combine_bwd_launch(int dtype, const void* g, const void* rows, int64_t num_rows, const int64_t* slots,
                           const float* weights, int64_t T, int K, int64_t width, void* g_rows, float* g_weights,
                           hipStream_t st) {
  if (int e = moe_dtype_ok(dtype)) return e;
  const int64_t row_bytes = width * elem_size(dtype);
  if (T < 0 || K < 1 || K > kMoeBwdMaxK || width < 1 || (row_bytes & 15) || num_rows < 1) return MP4X_E_BADARG;
  if (T == 0) return 0;
  if (T > INT32_MAX / 2 / K || !g || !rows || !g_rows || (((uintptr_t)g | (uintptr_t)rows | (uintptr_t)g_rows) & 15) ||
      !slots || ((uintptr_t)slots & 7) || !weights || ((uintptr_t)weights & 3) || !g_weights ||
      ((uintptr_t)g_weights & 3))
    return MP4X_E_BADARG;
  if (moe_overlap(g_rows, num_rows * row_bytes, rows, num_rows * row_bytes) ||
      moe_overlap(g_rows, num_rows * row_bytes, g, T * row_bytes))
    return MP4X_E_BADARG;
  const int64_t V = row_bytes / 16;
  const int G = lane_group(V);
  const int grid = grid_for((T * G + 63) / 64 * 64, 1);
  return with_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    if constexpr (DT == MP4X_F32 || DT == MP4X_BF16 || DT == MP4X_F16) {
      auto launch = [&](auto kmax) {
        hipLaunchKernelGGL((k_moe_combine_bwd<DT, decltype(kmax)::value>), dim3(grid), dim3(kBlock), 0, st,
                           (const u32x4*)g, (const u32x4*)rows, slots, weights, T, K, V, G, num_rows, (u32x4*)g_rows,
                           g_weights);
        return (int)hipGetLastError();
      };
      return K <= 4 ? launch(IntC<4>{}) : (K <= 8 ? launch(IntC<8>{}) : launch(IntC<kMoeBwdMaxK>{}));
    } else {
      return (int)MP4X_E_UNSUPPORTED;
    }
  });
}
}  // namespace

extern "C" int mp4x_moe_combine_backward(int dtype, const void* g, const void* rows, int64_t num_rows,
                                         const int64_t* slots, const float* weights, int64_t T, int K, int64_t width,
                                         void* g_rows, float* g_weights, void* stream) {
  return moe_combine_bwd_launch(dtype, g, rows, num_rows, slots, weights, T, K, width, g_rows, g_weights,
                                (hipStream_t)stream);
}

// K11 into the padded layout: the kernel writes the kept rows, the pad fill the rows [min(cnt[e],
// cap), cap) of every expert block from the scan the plan's route left in scratch.
extern "C" int mp4x_moe_combine_backward_pad(int dtype, const void* g, const void* rows, const int64_t* slots,
                                             const float* weights, int64_t T, int K, int64_t width, int64_t n, int nb,
                                             int64_t cap, void* scratch, size_t scratch_bytes, void* g_rows,
                                             float* g_weights, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int e = moe_dtype_ok(dtype)) return e;
  const int64_t row_bytes = width * elem_size(dtype);
  if (nb < 1 || nb > kMoeMaxNb || cap < 1 || cap > INT32_MAX / nb || T < 0 || K < 1 || K > kMoeBwdMaxK ||
      T > INT32_MAX / 2 / K || n != T * K || width < 1 || (row_bytes & 15) || !g_rows || ((uintptr_t)g_rows & 15))
    return MP4X_E_BADARG;
  if (n == 0) return moe_pad_fill_launch(nullptr, nb, cap, row_bytes / 16, g_rows, st);
  if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < mp4x_moe_route_scratch_bytes(n, nb)) return MP4X_E_BADARG;
  if (int e = moe_combine_bwd_launch(dtype, g, rows, (int64_t)nb * cap, slots, weights, T, K, width, g_rows, g_weights, st))
    return e;
  const MoeScratch S = moe_scratch(scratch, scratch_bytes, n, nb);
  return moe_pad_fill_launch(&S, nb, cap, row_bytes / 16, g_rows, st);
}
