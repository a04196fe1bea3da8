// K15 — drop by gate weight: the per-expert top-S select in front of K9's route (gfx950).
//
// out[a] = ids[a] for the limit[e] assignments of every expert e with the largest words
// (moe_prio_map.hpp: the gate weight's key, then the lower assignment index), -1 for the others of
// e; a negative id and an id >= nb pass through.  A dispatch on `out` is then the position policy's
// dispatch with nothing left to drop, so moe.hip's kernels run unchanged behind this file.
//
//   keys    k_moe_prio_keys    k_moe_scatter's ballot ranks without its row mover, over the scanned
//                              bases mp4x_moe_route_count left in its scratch: the word of every
//                              placed assignment goes to its slot of the stable sort by expert, so
//                              the words of an expert are one contiguous segment
//   select  k_moe_prio_select  a block per expert; an expert with cnt <= limit (or limit 0) writes
//                              its mode and returns.  Else 8 passes of the MSD radix select over the
//                              segment: a 256-bin LDS histogram of the pass's digit over the words
//                              that still carry the chosen prefix (integer LDS atomics), then thread 0
//                              walks the histogram from the top (prio::digit_step).  After 8 passes
//                              the prefix is the limit-th largest word itself.  8 * cnt word reads
//                              per selecting expert, whatever the ids are: no O(cnt^2) ranking
//   mask    k_moe_prio_mask    elementwise: the word again from (priority[a], a), the expert's mode
//                              and threshold, out[a]; the number it turned into -1 per block
//           k_moe_prio_sum     one block adds the per-block numbers: masked
//
// Integer atomics in LDS only, no floating-point arithmetic at all: identical run to run.  No host
// read, no allocation: the caller gives the scratch, so a call can be recorded in a graph.
#include "common.hpp"
#include "moe_prio_map.hpp"

namespace mp4x {

constexpr int kPrioMaxNb = 2048;     // moe.hip: kMoeMaxNb

__device__ __forceinline__ int64_t prio_id(const void* __restrict__ ids, int is_i64, int64_t i) {
  return is_i64 ? reinterpret_cast<const int64_t*>(ids)[i] : (int64_t)reinterpret_cast<const int32_t*>(ids)[i];
}

__global__ __launch_bounds__(kBlock) void k_moe_prio_keys(const void* __restrict__ ids, int is_i64,
                                                          const uint32_t* __restrict__ priority, int64_t n, int nb,
                                                          int64_t nblk, const int64_t* __restrict__ off,
                                                          uint64_t* __restrict__ words) {
  extern __shared__ __attribute__((aligned(16))) int32_t wcnt[];                // [4][nb]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t b = blockIdx.x, i = b * kBlock + tid;
  for (int j = tid; j < 4 * nb; j += kBlock) wcnt[j] = 0;
  __syncthreads();
  const int64_t id = i < n ? prio_id(ids, is_i64, i) : -1;
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
  if (placed) {
    int inb = rank;
    for (int q = 0; q < w; ++q) inb += wcnt[q * nb + d];
    const int64_t ps = off[(int64_t)d * nblk + b] + inb;
    // the scan is the same ids': ps < n always.  The guard costs a compare and keeps a scratch
    // that is not this call's route from becoming a store outside `words`
    if (ps >= 0 && ps < n) words[ps] = prio::word(priority[i], (uint32_t)i);
  }
}

// thr[2 * e] = the threshold word of expert e, thr[2 * e + 1] = its mode (prio::kAll / kSelect / kNone).
__global__ __launch_bounds__(kBlock) void k_moe_prio_select(const int64_t* __restrict__ off, int64_t nblk, int64_t n,
                                                            int64_t limit, const int64_t* __restrict__ limit_vec,
                                                            const uint64_t* __restrict__ words,
                                                            uint64_t* __restrict__ thr) {
  __shared__ uint32_t hist[prio::kBins];
  __shared__ uint64_t s_prefix;
  const int e = blockIdx.x, tid = threadIdx.x;
  int64_t lo = off[(int64_t)e * nblk], hi = off[(int64_t)(e + 1) * nblk];   // bucket e + 1 exists: nb + 2 buckets
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  const int64_t cnt = hi - lo;
  const int64_t L = limit_vec ? limit_vec[e] : limit;
  const int m = prio::mode(cnt, L);
  if (m != prio::kSelect) {              // block-uniform: before the first barrier
    if (tid == 0) {
      thr[2 * e] = 0;
      thr[2 * e + 1] = (uint64_t)m;
    }
    return;
  }
  const uint64_t* seg = words + lo;
  uint64_t prefix = 0, remaining = (uint64_t)L;      // 1 <= L < cnt here
  for (int pass = 0; pass < prio::kPasses; ++pass) {
    for (int j = tid; j < prio::kBins; j += kBlock) hist[j] = 0;
    __syncthreads();
    constexpr int UNR = 4;               // four independent 8-byte loads per lane in flight
    for (int64_t i0 = tid; i0 < cnt; i0 += (int64_t)kBlock * UNR) {
      uint64_t v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int64_t i = i0 + (int64_t)u * kBlock;
        v[u] = i < cnt ? seg[i] : 0;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u)
        if (i0 + (int64_t)u * kBlock < cnt && prio::candidate(v[u], prefix, pass))
          atomicAdd(&hist[prio::digit(v[u], pass)], 1u);
    }
    __syncthreads();
    if (tid == 0) s_prefix = (prefix << 8) | (uint64_t)prio::digit_step(hist, &remaining);
    __syncthreads();
    prefix = s_prefix;
  }
  if (tid == 0) {
    thr[2 * e] = prefix;
    thr[2 * e + 1] = (uint64_t)prio::kSelect;
  }
}

template <bool I64>
__global__ __launch_bounds__(kBlock) void k_moe_prio_mask(const void* __restrict__ ids,
                                                          const uint32_t* __restrict__ priority, int64_t n, int nb,
                                                          const uint64_t* __restrict__ thr, void* __restrict__ out,
                                                          int64_t* __restrict__ part) {
  __shared__ int32_t wsum[kBlock / 64];
  using T = std::conditional_t<I64, int64_t, int32_t>;
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  bool gone = false;
  if (i < n) {
    const T id = reinterpret_cast<const T*>(ids)[i];
    T o = id;
    if (id >= 0 && id < nb) {
      const uint64_t tau = thr[2 * (int64_t)id];
      const int m = (int)thr[2 * (int64_t)id + 1];
      gone = !prio::keeps(m, tau, prio::word(priority[i], (uint32_t)i));
      if (gone) o = (T)-1;
    }
    reinterpret_cast<T*>(out)[i] = o;
  }
  const int c = __popcll(__ballot(gone));
  if ((tid & 63) == 0) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int q = 0; q < kBlock / 64; ++q) s += wsum[q];
    part[blockIdx.x] = s;
  }
}

// One block: masked = the sum of the per-block numbers.  Integer sums: identical run to run.
__global__ __launch_bounds__(kBlock) void k_moe_prio_sum(const int64_t* __restrict__ part, int64_t nblk,
                                                         int64_t* __restrict__ masked) {
  __shared__ unsigned long long total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (int64_t b = threadIdx.x; b < nblk; b += kBlock) mine += (unsigned long long)part[b];
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0) masked[0] = (int64_t)total;
}

}  // namespace mp4x

using namespace mp4x;

namespace {
size_t prio_align(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

// words uint64[n] | thr uint64[2 * nb] | part int64[ceil(n / 256)], each 256-byte aligned.
extern "C" size_t mp4x_moe_priority_scratch_bytes(int64_t n, int nb) {
  if (n < 0 || n > INT32_MAX / 2 || nb < 1 || nb > kPrioMaxNb) return 0;
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  return prio_align((size_t)n * 8) + prio_align((size_t)nb * 16) + prio_align((size_t)(nblk < 1 ? 1 : nblk) * 8);
}

extern "C" int mp4x_moe_priority_mask(const void* ids, int ids_are_i64, const float* priority, int64_t n, int nb,
                                      int64_t limit, const int64_t* limit_vec, const void* route_scratch,
                                      size_t route_scratch_bytes, void* out_ids, int64_t* masked, void* scratch,
                                      size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (nb < 1 || nb > kPrioMaxNb || n < 0 || !masked || ((uintptr_t)masked & 7) || ((uintptr_t)limit_vec & 7) ||
      (!limit_vec && limit < 0))
    return MP4X_E_BADARG;
  if (n == 0) return (int)hipMemsetAsync(masked, 0, sizeof(int64_t), st);
  const int am = ids_are_i64 ? 7 : 3;
  if (n > INT32_MAX / 2 || !ids || ((uintptr_t)ids & am) || !out_ids || ((uintptr_t)out_ids & am) || !priority ||
      ((uintptr_t)priority & 3) || !route_scratch || ((uintptr_t)route_scratch & 255) || !scratch ||
      ((uintptr_t)scratch & 255) || out_ids == ids)
    return MP4X_E_BADARG;
  if (route_scratch_bytes < mp4x_moe_route_scratch_bytes(n, nb) || scratch_bytes < mp4x_moe_priority_scratch_bytes(n, nb))
    return MP4X_E_BADARG;
  // the route scratch as moe.hip lays it out: hist | off, (nb + 2) * nblk int64 each, 256-byte aligned
  const int64_t nblk = (n + kBlock - 1) / kBlock;
  const int64_t* off = (const int64_t*)((const char*)route_scratch + prio_align((size_t)(nb + 2) * nblk * sizeof(int64_t)));
  uint64_t* words = (uint64_t*)scratch;
  uint64_t* thr = (uint64_t*)((char*)scratch + prio_align((size_t)n * 8));
  int64_t* part = (int64_t*)((char*)thr + prio_align((size_t)nb * 16));
  const uint32_t* pbits = (const uint32_t*)priority;
  hipLaunchKernelGGL(k_moe_prio_keys, dim3(nblk), dim3(kBlock), 4 * nb * sizeof(int32_t), st, ids, ids_are_i64, pbits, n,
                     nb, nblk, off, words);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_moe_prio_select, dim3(nb), dim3(kBlock), 0, st, off, nblk, n, limit, limit_vec,
                     (const uint64_t*)words, thr);
  if (int e = (int)hipGetLastError()) return e;
  if (ids_are_i64)
    hipLaunchKernelGGL((k_moe_prio_mask<true>), dim3(nblk), dim3(kBlock), 0, st, ids, pbits, n, nb, (const uint64_t*)thr,
                       out_ids, part);
  else
    hipLaunchKernelGGL((k_moe_prio_mask<false>), dim3(nblk), dim3(kBlock), 0, st, ids, pbits, n, nb, (const uint64_t*)thr,
                       out_ids, part);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_moe_prio_sum, dim3(1), dim3(kBlock), 0, st, (const int64_t*)part, nblk, masked);
  return (int)hipGetLastError();
}
