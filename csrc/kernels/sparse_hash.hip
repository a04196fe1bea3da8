// K5h — hash reduce-by-key (gfx950): the opt-in alternative to the sort-based K5 of sparse.hip
// (MP4X_SPARSE_RBK=hash; VERDICT r5 Next #6).
//
// Reference hot loop: the MapReduce deserializer's per-key merge
// (/root/reference/src/main/java/com/fenbi/mp4j/operand/DoubleOperand.java:225-257) and the map
// branch of threadReduce (:458-477) — a HashMap<String, T> probe + combine per received entry.
// Here the keys are 64-bit ids and a map is (keys[n], rows[n][dim]).
//
// The sort path radix-sorts the full 64-bit keys (8 onesweep passes over keys + indices) to find
// the runs, then a run-start select and the segmented reduce.  The hash path needs four launches
// and no sort, no scan and no permutation arrays:
//
//   init     table keys <- EMPTY, slot list heads <- -1, the run counter <- 0 (one kernel)
//   insert   one lane per row: splitmix64 hash, linear probing, 64-bit CAS on an EMPTY slot
//            (table >= 2n slots, power of two: an empty slot always exists); the row is pushed on
//            its slot's list (one atomic exchange of the head; next[row] = the old head)
//   compact  4 slots per lane, one atomic per BLOCK (LDS prefix over the block's lanes): every
//            occupied slot gets a dense run index u; out_keys[u] and the run's list head
//   reduce   G lanes per run (a 16-byte vector each): one lane walks the run's list into LDS and
//            puts the row indices in ascending order (runs up to 64 rows), then the group combines
//            the rows in that order (= input = rank order): the same values, bit for bit, as the
//            sort path, which also combines in input order
//
// Differences from the sort path (why K5h stays opt-in): the output keys come in table order,
// which depends on which of two colliding keys' CAS wins, not ascending; a run longer than 64
// rows combines in list order (float SUM / PROD of such a key is then not bit-reproducible;
// integer data and MAX / MIN are exact either way); the FIRST rule (K8) is not served.  Rows
// whose key equals -1 (the EMPTY marker) form a side run of their own.
//
// K5c (mp4x_hash_reduce_by_key_canonical) is the hash path with those differences removed, for a
// caller that needs the output to be a function of the input: the table is the CANONICAL one
// (sparse_hash_map.hpp: plain linear probing of the distinct keys in ascending unsigned order,
// reached from any insertion order by priority insertion, k_hashc_insert), the rows are linked
// by a second, read-only probe when the table is final (k_hashc_link), the runs are numbered in
// slot order by K5d's count / scan / compact (no atomic on the run counter; the -1 run last),
// and every run, however long, combines in ascending row index.  Every loop is bounded; a lane
// past a bound sets m_flag[1] and the caller takes the sort path.
//
// K5d (below) is the identity-hash form for DENSE keys (k / stride - base in [0, T)): no
// probing, an ordered compaction, so the keys come out ascending — the sort path's result and
// order — and the tensor forms take it by default where the carried key range allows.
#include <rocprim/device/device_scan.hpp>
#include <type_traits>

#include "common.hpp"
#include "sparse_hash_map.hpp"

namespace mp4x {

namespace {
using hmap::hash_mix;
using hmap::table_slots;
constexpr unsigned long long kHashEmpty = hmap::kEmpty;
constexpr int kCompactPer = 4;             // slots per lane in k_hash_compact (>= 2 blocks per CU at 2n = 400k)
constexpr int kOrderMax = 64;              // longest run whose rows are put in input order

// The side run of rows keyed -1 (the EMPTY marker): its list head and, once compacted, its run.
struct SideRun {
  int32_t head;
  int32_t u;
};

__global__ __launch_bounds__(kBlock) void k_hash_init(unsigned long long* __restrict__ tkeys,
                                                      int32_t* __restrict__ thead, int64_t nslots,
                                                      SideRun* __restrict__ side, unsigned long long* __restrict__ m_flag) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t0 == 0) {
    side->head = -1;
    side->u = -1;
    m_flag[0] = 0;
    m_flag[1] = 0;
  }
  for (int64_t h = t0; h < nslots; h += nthr) {
    tkeys[h] = kHashEmpty;
    thead[h] = -1;
  }
}

__global__ __launch_bounds__(kBlock) void k_hash_insert(const int64_t* __restrict__ keys, int64_t n,
                                                        unsigned long long* __restrict__ tkeys,
                                                        int32_t* __restrict__ thead, uint64_t mask,
                                                        int32_t* __restrict__ next, SideRun* __restrict__ side) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthr) {
    const unsigned long long k = (unsigned long long)keys[i];
    int32_t* head = &side->head;
    if (k != kHashEmpty) {
      uint64_t h = hash_mix(k) & mask;
      for (;;) {
        unsigned long long cur = __hip_atomic_load(&tkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kHashEmpty) {
          cur = atomicCAS(&tkeys[h], kHashEmpty, k);
          if (cur == kHashEmpty) cur = k;                // inserted here
        }
        if (cur == k) break;
        h = (h + 1) & mask;
      }
      head = &thead[h];
    }
    next[i] = atomicExch(head, (int32_t)i);              // push row i on its run's list
  }
}

// ---------------------------------------------------------------- K5c: the canonical table
// The table as a function of the key SET (sparse_hash_map.hpp): priority linear probing, the
// smaller unsigned key wins a slot and the displaced key moves on.  No row lists here: a row's
// slot is final only when every row is in.  A lane past one of the header's two bounds sets
// m_flag[1] and stops (the caller then takes the sort path): nothing spins without a bound.
__global__ __launch_bounds__(kBlock) void k_hashc_insert(const int64_t* __restrict__ keys, int64_t n,
                                                         unsigned long long* __restrict__ tkeys, uint64_t mask,
                                                         uint64_t max_advance, uint64_t max_iter,
                                                         unsigned long long* __restrict__ m_flag) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthr) {
    unsigned long long v = (unsigned long long)keys[i];
    if (v == kHashEmpty) continue;                       // the side run: k_hashc_link
    uint64_t h = hmap::home(v, mask);
    uint64_t adv = 0, it = 0;
    unsigned long long c = __hip_atomic_load(&tkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
      if (++it > max_iter) {
        atomicOr(&m_flag[1], 1ull);
        break;
      }
      const int act = hmap::step(c, v);
      if (act == hmap::kDone) break;
      if (act == hmap::kSwap) {
        const unsigned long long old = atomicCAS(&tkeys[h], c, v);
        if (old != c) {                                  // lost: step again on the slot's new value
          c = old;
          continue;
        }
        if (c == kHashEmpty) break;                      // took an empty slot: nothing to carry on
        v = c;                                           // the displaced key moves on
      }
      if (++adv >= max_advance) {
        atomicOr(&m_flag[1], 1ull);
        break;
      }
      h = (h + 1) & mask;
      c = __hip_atomic_load(&tkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// A launch of its own, when the table is final: every row finds its key's slot by a read-only
// probe from the key's home (at most max_advance slots; an empty slot or the bound means the
// insert gave up: m_flag[1]) and is pushed on the slot's list.  Rows keyed -1: the side run.
__global__ __launch_bounds__(kBlock) void k_hashc_link(const int64_t* __restrict__ keys, int64_t n,
                                                       const unsigned long long* __restrict__ tkeys,
                                                       int32_t* __restrict__ thead, uint64_t mask,
                                                       uint64_t max_advance, int32_t* __restrict__ next,
                                                       SideRun* __restrict__ side,
                                                       unsigned long long* __restrict__ m_flag) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthr) {
    const unsigned long long k = (unsigned long long)keys[i];
    int32_t* head = &side->head;
    if (k != kHashEmpty) {
      uint64_t h = hmap::home(k, mask);
      uint64_t adv = 0;
      unsigned long long cur = tkeys[h];
      while (cur != k && cur != kHashEmpty && ++adv < max_advance) {
        h = (h + 1) & mask;
        cur = tkeys[h];
      }
      if (cur != k) {                                    // not in the table
        atomicOr(&m_flag[1], 1ull);
        next[i] = -1;
        continue;
      }
      head = &thead[h];
    }
    next[i] = atomicExch(head, (int32_t)i);              // push row i on its run's list
  }
}

// A tile of kBlock * kCompactPer slots per block (slot = tile + j * kBlock + lane, coalesced);
// the block's occupied slots take consecutive run indices from ONE atomic on the run counter.
__global__ __launch_bounds__(kBlock) void k_hash_compact(const unsigned long long* __restrict__ tkeys,
                                                         const int32_t* __restrict__ thead, int64_t nslots,
                                                         int64_t* __restrict__ out_keys, int32_t* __restrict__ rhead,
                                                         unsigned long long* __restrict__ counter,
                                                         const SideRun* __restrict__ side) {
  __shared__ int s_pre[kBlock];
  __shared__ unsigned long long s_base;
  if (blockIdx.x == 0 && threadIdx.x == 0 && side->head >= 0) {     // the side run, if any
    const int64_t u = (int64_t)atomicAdd(counter, 1ull);
    out_keys[u] = -1;
    rhead[u] = side->head;
  }
  const int64_t tile = (int64_t)blockIdx.x * kBlock * kCompactPer;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kCompactPer; ++j) {
    const int64_t h = tile + (int64_t)j * kBlock + threadIdx.x;
    mine += (h < nslots && tkeys[h] != kHashEmpty) ? 1 : 0;
  }
  s_pre[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {           // inclusive Hillis-Steele scan in LDS
    const int v = threadIdx.x >= off ? s_pre[threadIdx.x - off] : 0;
    __syncthreads();
    s_pre[threadIdx.x] += v;
    __syncthreads();
  }
  if (threadIdx.x == kBlock - 1) s_base = s_pre[kBlock - 1] ? atomicAdd(counter, (unsigned long long)s_pre[kBlock - 1]) : 0;
  __syncthreads();
  int64_t u = (int64_t)s_base + s_pre[threadIdx.x] - mine;
#pragma unroll
  for (int j = 0; j < kCompactPer; ++j) {
    const int64_t h = tile + (int64_t)j * kBlock + threadIdx.x;
    if (h < nslots) {
      const unsigned long long k = tkeys[h];
      if (k != kHashEmpty) {
        out_keys[u] = (int64_t)k;
        rhead[u] = thead[h];
        ++u;
      }
    }
  }
}

// LDS written by one lane, read by the others of its wave: complete the writes, keep the compiler
// from moving LDS accesses across (no s_barrier: the groups of a block diverge).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kMinG = 4;                   // lanes per run at least (bounds the LDS index lists)

// G lanes per run, 64 / G runs per wave.  Unit = a 16-byte vector of W elements (VEC) or one
// element; `units` per row.  Lane 0 of a group walks the run's list into its LDS list (ascending
// insertion: runs up to kOrderMax rows), the group combines the rows in that order, two in flight.
// A longer run combines in list order (walking the list again) — or, with ORDERED (K5c), in
// ascending row index as well, in batches of kOrderMax rows: for every batch the walker walks the
// list once more and keeps the kOrderMax smallest indices above the previous batch's largest (the
// same sorted insertion), O(L^2 / kOrderMax) list steps for a run of L rows.
template <int DT, int OP, bool VEC, bool ORDERED = false>
__global__ __launch_bounds__(kBlock) void k_hash_reduce(const int32_t* __restrict__ rhead,
                                                        const int32_t* __restrict__ next,
                                                        const unsigned long long* __restrict__ m_dev,
                                                        const void* __restrict__ vals_, int64_t units, int G,
                                                        void* __restrict__ out_, int32_t* __restrict__ out_count) {
  using S = typename Elem<DT>::S;
  using A = typename Elem<DT>::A;
  using U = typename std::conditional<VEC, u32x4, S>::type;   // a row's unit: 16 bytes, or one element
  constexpr int W = VEC ? 16 / (int)sizeof(S) : 1;
  __shared__ int32_t s_idx[kBlock / kMinG][kOrderMax];
  const U* vals = reinterpret_cast<const U*>(vals_);
  U* out = reinterpret_cast<U*>(out_);
  const int lane = threadIdx.x & 63;
  const int grp = lane / G, sub = lane % G, R = 64 / G;
  int32_t* buf = s_idx[(threadIdx.x >> 6) * R + grp];
  const int64_t m = (int64_t)*m_dev;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
  for (int64_t u0 = wave * R; u0 < m; u0 += nwaves * R) {
    const int64_t u = u0 + grp;
    const bool live = u < m;
    int L = 0;
    if (live) {
      const int32_t h0 = rhead[u];
      if (sub == 0) {                                    // the walk, sorted insertion
        for (int32_t i = h0; i >= 0; i = next[i]) {
          if (L < kOrderMax) {
            int b = L - 1;
            while (b >= 0 && buf[b] > i) {
              buf[b + 1] = buf[b];
              --b;
            }
            buf[b + 1] = i;
          }
          ++L;
        }
      }
    }
    wave_lds_sync();
    L = __shfl(L, lane - sub, 64);                      // the group's walker has the length
    if (!live) continue;
    if (sub == 0 && out_count) out_count[u] = L;
    const bool listed = L <= kOrderMax;
    for (int64_t v = sub; v < units; v += G) {
      A acc[W];
      auto row = [&](int32_t i) { return vals[(int64_t)i * units + v]; };
      if (listed) {
        unpack<DT>(row(buf[0]), acc);
        int j = 1;
        for (; j + 1 < L; j += 2) {                      // two rows in flight
          const U t0 = row(buf[j]);
          const U t1 = row(buf[j + 1]);
          fold_in<DT, OP>(acc, t0);
          fold_in<DT, OP>(acc, t1);
        }
        if (j < L) fold_in<DT, OP>(acc, row(buf[j]));
      } else if constexpr (ORDERED) {
        // L, v - sub and so every trip count below are the same in all lanes of the group
        int32_t prev = -1;                               // the largest row index combined so far
        for (int done = 0; done < L; done += kOrderMax) {
          const int cnt = L - done < kOrderMax ? L - done : kOrderMax;
          wave_lds_sync();                               // the group has read the previous batch
          if (sub == 0) {
            int have = 0, s = 0;
            for (int32_t i = rhead[u]; i >= 0 && s < L; i = next[i], ++s) {
              if (i <= prev || (have == kOrderMax && i > buf[kOrderMax - 1])) continue;
              int b = (have < kOrderMax ? have : kOrderMax - 1) - 1;
              while (b >= 0 && buf[b] > i) {
                buf[b + 1] = buf[b];
                --b;
              }
              buf[b + 1] = i;
              if (have < kOrderMax) ++have;
            }
          }
          wave_lds_sync();
          int j = 0;
          if (done == 0) unpack<DT>(row(buf[j++]), acc);
          for (; j < cnt; ++j) fold_in<DT, OP>(acc, row(buf[j]));
          prev = buf[cnt - 1];
        }
      } else {
        int32_t i = rhead[u];
        unpack<DT>(row(i), acc);
        for (i = next[i]; i >= 0; i = next[i]) fold_in<DT, OP>(acc, row(i));
      }
      out[u * units + v] = pack<DT, U>(acc);
    }
  }
}

// ---------------------------------------------------------------- K5d: dense keys
// When the keys of a reduce-by-key are dense — k / stride - base in [0, T) with T a small multiple
// of n (dictionary ids; an owner's share of them, stride = p) — the hash is the identity: no
// probing, and the occupied slots in slot order ARE the keys in ascending order.  The same row
// lists and in-order reduce as K5h, so the output is the sort path's, bit for bit and in the same
// (ascending) key order.  A key outside [0, T) or two keys on one slot set m_flag[1]: the caller
// falls back to the sort path.
__global__ __launch_bounds__(kBlock) void k_dense_init(unsigned long long* __restrict__ tkeys,
                                                       int32_t* __restrict__ thead, int64_t T,
                                                       unsigned long long* __restrict__ m_flag) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t0 == 0) {
    m_flag[0] = 0;
    m_flag[1] = 0;
  }
  for (int64_t h = t0; h < T; h += nthr) {
    tkeys[h] = kHashEmpty;
    thead[h] = -1;
  }
}

__global__ __launch_bounds__(kBlock) void k_dense_insert(const int64_t* __restrict__ keys, int64_t n, int64_t base,
                                                         int64_t stride, int64_t T,
                                                         unsigned long long* __restrict__ tkeys,
                                                         int32_t* __restrict__ thead, int32_t* __restrict__ next,
                                                         unsigned long long* __restrict__ m_flag) {
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += nthr) {
    const int64_t k = keys[i];
    const int64_t h = k >= 0 ? k / stride - base : -1;
    if (h < 0 || h >= T) {                               // not dense after all
      atomicOr(&m_flag[1], 1ull);
      next[i] = -1;
      continue;
    }
    const unsigned long long cur = atomicCAS(&tkeys[h], kHashEmpty, (unsigned long long)k);
    if (cur != kHashEmpty && cur != (unsigned long long)k) atomicOr(&m_flag[1], 1ull);   // two keys, one slot
    next[i] = atomicExch(&thead[h], (int32_t)i);
  }
}

// Tiles of kBlock * kCompactPer consecutive slots, kCompactPer consecutive slots per lane (so
// the dense run index follows the slot order): the occupied count of every tile.
__global__ __launch_bounds__(kBlock) void k_dense_count(const int32_t* __restrict__ thead, int64_t T,
                                                        int64_t* __restrict__ tile_cnt) {
  __shared__ int s_sum[kBlock / 64];
  const int64_t h0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer;
  int c = 0;
#pragma unroll
  for (int j = 0; j < kCompactPer; ++j) c += (h0 + j < T && thead[h0 + j] >= 0) ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int q = 0; q < kBlock / 64; ++q) t += s_sum[q];
    tile_cnt[blockIdx.x] = t;
  }
}

// Dense run indices in slot order: the tile's base (scanned) + the lane prefix in LDS.
__global__ __launch_bounds__(kBlock) void k_dense_compact(const unsigned long long* __restrict__ tkeys,
                                                          const int32_t* __restrict__ thead, int64_t T,
                                                          const int64_t* __restrict__ tile_base,
                                                          const int64_t* __restrict__ tile_cnt, int64_t ntiles,
                                                          int64_t* __restrict__ out_keys,
                                                          int32_t* __restrict__ rhead,
                                                          unsigned long long* __restrict__ m_flag) {
  __shared__ int s_pre[kBlock];
  const int64_t h0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer;
  int mine = 0;
#pragma unroll
  for (int j = 0; j < kCompactPer; ++j) mine += (h0 + j < T && thead[h0 + j] >= 0) ? 1 : 0;
  s_pre[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {           // inclusive Hillis-Steele scan in LDS
    const int v = threadIdx.x >= off ? s_pre[threadIdx.x - off] : 0;
    __syncthreads();
    s_pre[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t u = tile_base[blockIdx.x] + s_pre[threadIdx.x] - mine;
#pragma unroll
  for (int j = 0; j < kCompactPer; ++j) {
    const int64_t h = h0 + j;
    if (h < T) {
      const int32_t hd = thead[h];
      if (hd >= 0) {
        out_keys[u] = (int64_t)tkeys[h];
        rhead[u] = hd;
        ++u;
      }
    }
  }
  if (blockIdx.x == ntiles - 1 && threadIdx.x == 0)
    m_flag[0] = (unsigned long long)(tile_base[ntiles - 1] + tile_cnt[ntiles - 1]);
}

// K5c: the side run of rows keyed -1, if any, becomes the last run.  One lane, after
// k_dense_compact has written m_flag[0]: no atomic on the run counter.
__global__ void k_hashc_side(const SideRun* __restrict__ side, int64_t* __restrict__ out_keys,
                             int32_t* __restrict__ rhead, unsigned long long* __restrict__ m_flag) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || side->head < 0) return;
  const unsigned long long u = m_flag[0];
  out_keys[u] = -1;
  rhead[u] = side->head;
  m_flag[0] = u + 1;
}

// Keys only (set operations): every run's row count, one lane per run walking its list.
__global__ __launch_bounds__(kBlock) void k_run_counts(const int32_t* __restrict__ rhead,
                                                       const int32_t* __restrict__ next,
                                                       const unsigned long long* __restrict__ m_dev,
                                                       int32_t* __restrict__ out_count) {
  const int64_t m = (int64_t)*m_dev;
  const int64_t nthr = (int64_t)gridDim.x * kBlock;
  for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < m; u += nthr) {
    int32_t L = 0;
    for (int32_t i = rhead[u]; i >= 0; i = next[i]) ++L;
    out_count[u] = L;
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The scratch layout (every part 256-byte aligned): table keys, slot list heads, next[row],
// run list heads, the side run.
struct Layout {
  size_t tkeys, thead, next, rhead, side, total;
  int64_t t;
};

Layout layout(int64_t n) {
  Layout L;
  L.t = table_slots(n);
  size_t o = 0;
  L.tkeys = o;  o += align256((size_t)L.t * 8);
  L.thead = o;  o += align256((size_t)L.t * 4);
  L.next = o;   o += align256((size_t)n * 4);
  L.rhead = o;  o += align256((size_t)n * 4);
  L.side = o;   o += 256;
  L.total = o;
  return L;
}

template <int DT, int OP, bool ORDERED>
int launch_reduce(const int32_t* rhead, const int32_t* next, const unsigned long long* m_dev, int64_t n,
                  const void* vals, int64_t dim, void* out, int32_t* out_count, hipStream_t st) {
  using S = typename Elem<DT>::S;
  const int64_t row_bytes = dim * (int64_t)sizeof(S);
  const bool vec = (row_bytes & 15) == 0 && ((((uintptr_t)vals | (uintptr_t)out) & 15) == 0);
  const int64_t units = vec ? row_bytes / 16 : dim;
  int G = kMinG;
  while (G < units && G < 64) G <<= 1;
  const int g = grid_for((n * G + 63) / 64 * 64, 1);
  if (vec)
    hipLaunchKernelGGL((k_hash_reduce<DT, OP, true, ORDERED>), dim3(g), dim3(kBlock), 0, st, rhead, next, m_dev, vals, units,
                       G, out, out_count);
  else
    hipLaunchKernelGGL((k_hash_reduce<DT, OP, false, ORDERED>), dim3(g), dim3(kBlock), 0, st, rhead, next, m_dev, vals, units,
                       G, out, out_count);
  return (int)hipGetLastError();
}

// The reduce launch of the entry points (hash, dense, canonical), for a runtime (dtype, op).
// ``ordered``: runs longer than kOrderMax rows combine in input order too (K5c).
int reduce_runs(int dtype, int op, const int32_t* rhead, const int32_t* next, const unsigned long long* m_dev,
                int64_t n, const void* vals, int64_t dim, void* out, int32_t* out_count, hipStream_t st,
                bool ordered = false) {
  return with_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    return with_op_of<DT>(RowOps{}, op, MP4X_E_UNSUPPORTED, [&](auto opc) {
      constexpr int OP = decltype(opc)::value;
      if (ordered) return launch_reduce<DT, OP, true>(rhead, next, m_dev, n, vals, dim, out, out_count, st);
      return launch_reduce<DT, OP, false>(rhead, next, m_dev, n, vals, dim, out, out_count, st);
    });
  });
}
}  // namespace

}  // namespace mp4x

namespace mp4x {
namespace {
struct DenseLayout {
  size_t tkeys, thead, next, rhead, tcnt, tbase, temp, total, temp_bytes;
  int64_t ntiles;
};

DenseLayout dense_layout(int64_t n, int64_t T) {
  DenseLayout L;
  const int64_t tile = (int64_t)kBlock * kCompactPer;
  L.ntiles = (T + tile - 1) / tile;
  size_t o = 0;
  L.tkeys = o;  o += align256((size_t)T * 8);
  L.thead = o;  o += align256((size_t)T * 4);
  L.next = o;   o += align256((size_t)n * 4);
  L.rhead = o;  o += align256((size_t)(n < T ? n : T) * 4);
  L.tcnt = o;   o += align256((size_t)L.ntiles * 8);
  L.tbase = o;  o += align256((size_t)L.ntiles * 8);
  L.temp_bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, L.temp_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0,
                                (size_t)(L.ntiles < 1 ? 1 : L.ntiles), rocprim::plus<int64_t>(), (hipStream_t)0);
  L.temp = o;   o += align256(L.temp_bytes);
  L.total = o;
  return L;
}

// K5c's scratch: the dense layout over T = table_slots(n) slots (table keys, slot list heads,
// next[row], run list heads, the tile counts and bases, the scan's temporary), then the side run.
struct CanonLayout {
  DenseLayout d;
  size_t side, total;
  int64_t t;
};

CanonLayout canon_layout(int64_t n) {
  CanonLayout L;
  L.t = table_slots(n);
  L.d = dense_layout(n, L.t);
  // (the dense layout's min(n, T) = n run list heads suffice: n rows give at most n runs, the side
  // run among them)
  L.side = L.d.total;
  L.total = L.side + 256;
  return L;
}
}  // namespace
}  // namespace mp4x

using namespace mp4x;

extern "C" size_t mp4x_hash_rbk_scratch_bytes(int64_t n) { return layout(n < 0 ? 0 : n).total; }

extern "C" int mp4x_hash_rbk_supported(int dtype, int op) { return pair_supported(RowOps{}, dtype, op) == 0; }

extern "C" int mp4x_hash_reduce_by_key(int dtype, int op, const int64_t* keys, int64_t n, const void* vals, int64_t dim,
                                       void* scratch, size_t scratch_bytes, int64_t* out_keys, void* out_vals,
                                       int32_t* out_count, int64_t* m_flag, void* stream) {
  if (!mp4x_hash_rbk_supported(dtype, op) || n < 0 || dim <= 0 || n >= (1ll << 30)) return MP4X_E_UNSUPPORTED;
  const Layout L = layout(n);
  if (scratch_bytes < L.total || ((uintptr_t)scratch & 255) || ((uintptr_t)m_flag & 7)) return MP4X_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)scratch;
  auto* tkeys = (unsigned long long*)(p + L.tkeys);
  auto* thead = (int32_t*)(p + L.thead);
  auto* next = (int32_t*)(p + L.next);
  auto* rhead = (int32_t*)(p + L.rhead);
  auto* side = (SideRun*)(p + L.side);
  auto* counter = (unsigned long long*)m_flag;            // m_flag[0]: the run counter IS m
  hipLaunchKernelGGL(k_hash_init, dim3(grid_for(L.t, 2)), dim3(kBlock), 0, st, tkeys, thead, L.t, side, counter);
  if (n == 0) return (int)hipGetLastError();
  hipLaunchKernelGGL(k_hash_insert, dim3(grid_for(n, 1)), dim3(kBlock), 0, st, keys, n, tkeys, thead,
                     (uint64_t)(L.t - 1), next, side);
  const int64_t tile = (int64_t)kBlock * kCompactPer;
  hipLaunchKernelGGL(k_hash_compact, dim3((unsigned)((L.t + tile - 1) / tile)), dim3(kBlock), 0, st,
                     (const unsigned long long*)tkeys, (const int32_t*)thead, L.t, out_keys, rhead, counter,
                     (const SideRun*)side);
  if (int e = (int)hipGetLastError()) return e;
  const unsigned long long* m_dev = counter;
  return reduce_runs(dtype, op, rhead, next, m_dev, n, vals, dim, out_vals, out_count, st);
}

extern "C" size_t mp4x_dense_rbk_scratch_bytes(int64_t n, int64_t T) {
  return dense_layout(n < 0 ? 0 : n, T < 1 ? 1 : T).total;
}

extern "C" int mp4x_dense_reduce_by_key(int dtype, int op, const int64_t* keys, int64_t n, const void* vals,
                                        int64_t dim, int64_t base, int64_t stride, int64_t T, void* scratch,
                                        size_t scratch_bytes, int64_t* out_keys, void* out_vals, int32_t* out_count,
                                        int64_t* m_flag, void* stream) {
  if ((vals && (!mp4x_hash_rbk_supported(dtype, op) || dim <= 0)) || n <= 0 || n >= (1ll << 30) || T < 1 ||
      T >= (1ll << 31) || stride < 1 || base < 0)
    return MP4X_E_UNSUPPORTED;
  const DenseLayout L = dense_layout(n, T);
  if (scratch_bytes < L.total || ((uintptr_t)scratch & 255) || ((uintptr_t)m_flag & 7)) return MP4X_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)scratch;
  auto* tkeys = (unsigned long long*)(p + L.tkeys);
  auto* thead = (int32_t*)(p + L.thead);
  auto* next = (int32_t*)(p + L.next);
  auto* rhead = (int32_t*)(p + L.rhead);
  auto* tcnt = (int64_t*)(p + L.tcnt);
  auto* tbase = (int64_t*)(p + L.tbase);
  auto* flag = (unsigned long long*)m_flag;
  hipLaunchKernelGGL(k_dense_init, dim3(grid_for(T, 2)), dim3(kBlock), 0, st, tkeys, thead, T, flag);
  hipLaunchKernelGGL(k_dense_insert, dim3(grid_for(n, 1)), dim3(kBlock), 0, st, keys, n, base, stride, T, tkeys, thead,
                     next, flag);
  hipLaunchKernelGGL(k_dense_count, dim3((unsigned)L.ntiles), dim3(kBlock), 0, st, (const int32_t*)thead, T, tcnt);
  size_t tb = L.temp_bytes;
  if (hipError_t e = rocprim::exclusive_scan(p + L.temp, tb, (const int64_t*)tcnt, tbase, (int64_t)0, (size_t)L.ntiles,
                                             rocprim::plus<int64_t>(), st))
    return (int)e;
  hipLaunchKernelGGL(k_dense_compact, dim3((unsigned)L.ntiles), dim3(kBlock), 0, st, (const unsigned long long*)tkeys,
                     (const int32_t*)thead, T, (const int64_t*)tbase, (const int64_t*)tcnt, L.ntiles, out_keys, rhead,
                     flag);
  if (int e = (int)hipGetLastError()) return e;
  const unsigned long long* m_dev = flag;
  if (!vals) {                                           // keys only: unique keys + counts
    if (!out_count) return 0;
    hipLaunchKernelGGL(k_run_counts, dim3(grid_for(n, 1)), dim3(kBlock), 0, st, (const int32_t*)rhead,
                       (const int32_t*)next, m_dev, out_count);
    return (int)hipGetLastError();
  }
  return reduce_runs(dtype, op, rhead, next, m_dev, n, vals, dim, out_vals, out_count, st);
}

extern "C" size_t mp4x_hash_rbk_canonical_scratch_bytes(int64_t n) { return canon_layout(n < 0 ? 0 : n).total; }

// K5c: init, priority insert, link (the table is final), ordered compaction over the table's slots
// (K5d's count / scan / compact), the side run last, the reduce with every run in input order.
extern "C" int mp4x_hash_reduce_by_key_canonical(int dtype, int op, const int64_t* keys, int64_t n, const void* vals,
                                                 int64_t dim, void* scratch, size_t scratch_bytes, int64_t* out_keys,
                                                 void* out_vals, int32_t* out_count, int64_t* m_flag, void* stream) {
  if (!mp4x_hash_rbk_supported(dtype, op) || n < 0 || dim <= 0 || n >= (1ll << 30)) return MP4X_E_UNSUPPORTED;
  const CanonLayout L = canon_layout(n);
  if (scratch_bytes < L.total || ((uintptr_t)scratch & 255) || ((uintptr_t)m_flag & 7)) return MP4X_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  char* p = (char*)scratch;
  auto* tkeys = (unsigned long long*)(p + L.d.tkeys);
  auto* thead = (int32_t*)(p + L.d.thead);
  auto* next = (int32_t*)(p + L.d.next);
  auto* rhead = (int32_t*)(p + L.d.rhead);
  auto* tcnt = (int64_t*)(p + L.d.tcnt);
  auto* tbase = (int64_t*)(p + L.d.tbase);
  auto* side = (SideRun*)(p + L.side);
  auto* flag = (unsigned long long*)m_flag;
  const uint64_t mask = (uint64_t)(L.t - 1);
  hipLaunchKernelGGL(k_hash_init, dim3(grid_for(L.t, 2)), dim3(kBlock), 0, st, tkeys, thead, L.t, side, flag);
  if (n == 0) return (int)hipGetLastError();
  hipLaunchKernelGGL(k_hashc_insert, dim3(grid_for(n, 1)), dim3(kBlock), 0, st, keys, n, tkeys, mask,
                     hmap::advance_bound(L.t), hmap::iter_bound(n, L.t), flag);
  hipLaunchKernelGGL(k_hashc_link, dim3(grid_for(n, 1)), dim3(kBlock), 0, st, keys, n,
                     (const unsigned long long*)tkeys, thead, mask, hmap::advance_bound(L.t), next, side, flag);
  hipLaunchKernelGGL(k_dense_count, dim3((unsigned)L.d.ntiles), dim3(kBlock), 0, st, (const int32_t*)thead, L.t, tcnt);
  size_t tb = L.d.temp_bytes;
  if (hipError_t e = rocprim::exclusive_scan(p + L.d.temp, tb, (const int64_t*)tcnt, tbase, (int64_t)0,
                                             (size_t)L.d.ntiles, rocprim::plus<int64_t>(), st))
    return (int)e;
  hipLaunchKernelGGL(k_dense_compact, dim3((unsigned)L.d.ntiles), dim3(kBlock), 0, st,
                     (const unsigned long long*)tkeys, (const int32_t*)thead, L.t, (const int64_t*)tbase,
                     (const int64_t*)tcnt, L.d.ntiles, out_keys, rhead, flag);
  hipLaunchKernelGGL(k_hashc_side, dim3(1), dim3(64), 0, st, (const SideRun*)side, out_keys, rhead, flag);
  if (int e = (int)hipGetLastError()) return e;
  return reduce_runs(dtype, op, rhead, next, flag, n, vals, dim, out_vals, out_count, st, true);
}
