// The table of the hash reduce-by-key (K5h, K5c of sparse_hash.hip): the hash, the table size, and
// the rule and loop bounds of the canonical (priority) insertion.  Plain C++ (no HIP types), the same
// code on the host and on the device: csrc/kernels/test_sparse_hash_map.cpp runs the insertion on
// the CPU, from shuffled orders and interleaved lanes, against the definition.
//
//   table_slots(n)  t = the smallest power of two >= max(1024, 2n) for n ROWS: at least t/2 slots
//                   stay empty whatever the keys
//   home(k, mask)   splitmix64(k) & (t - 1)
//   canonical table the result of plain linear probing when the distinct keys other than kEmpty are
//                   inserted in ascending UNSIGNED order.  It depends on the key set only.
//   step(c, v)      one step of a lane that carries key v and has read c from its slot: priority
//                   linear probing, "the smaller unsigned key wins", kEmpty (all ones) loses to every
//                   key.  kDone: v is here.  kAdvance: the slot keeps c < v, go to the next slot.
//                   kSwap: CAS c -> v; on success the lane carries c on from the next slot (and is
//                   done when c was kEmpty), on failure it takes the slot's new value as c and steps
//                   again.  From any insertion order and any interleaving of these steps the table
//                   ends as the canonical table (the phase-concurrent deterministic table of Shun
//                   and Blelloch, SPAA 2014).
//
// Bounds of one lane (n rows, t slots); a lane that passes one has met a broken table and gives up:
//   advance_bound(t) = t        slots advanced.  A legitimate probe ends at an empty slot or at its
//                               key after fewer than t/2 + 1 advances.
//   iter_bound(n, t)            steps in all = t + 1 + n (n + 1) / 2.  A step is the final one, an
//                               advance (a successful swap advances too: <= t together), or a failed
//                               CAS.  A CAS fails only when another lane's CAS on that slot succeeded
//                               between this lane's read and its CAS, and distinct failures of one
//                               lane have disjoint read-to-CAS windows, so a lane fails at most as
//                               often as CASes succeed in the whole launch.  A slot's value only
//                               decreases, so it takes a key at most once; and key k is only ever
//                               written between home(k) and its canonical slot (when k is written at
//                               slot i every slot from home(k) to i - 1 holds a smaller key for good,
//                               so the canonical slot of k cannot lie before i): at most d_k + 1
//                               successes write k, d_k its canonical displacement.  The j-th key of
//                               the ascending insertion skips at most j - 1 slots, so the successes
//                               number at most sum (d_k + 1) <= n (n + 1) / 2.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MP4X_HMAP_HD __host__ __device__ __forceinline__
#else
#define MP4X_HMAP_HD inline
#endif

namespace mp4x {
namespace hmap {

constexpr uint64_t kEmpty = ~0ull;

MP4X_HMAP_HD uint64_t hash_mix(uint64_t k) {   // splitmix64 finalizer
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  k ^= k >> 31;
  return k;
}

MP4X_HMAP_HD int64_t table_slots(int64_t n) {
  int64_t t = 1024;
  while (t < 2 * n) t <<= 1;
  return t;
}

MP4X_HMAP_HD uint64_t home(uint64_t k, uint64_t mask) { return hash_mix(k) & mask; }

enum : int { kDone = 0, kAdvance = 1, kSwap = 2 };

MP4X_HMAP_HD int step(uint64_t c, uint64_t v) { return c == v ? kDone : (c < v ? kAdvance : kSwap); }

MP4X_HMAP_HD uint64_t advance_bound(int64_t t) { return (uint64_t)t; }

// n < 2^30 (the entry points refuse more rows): no overflow.
MP4X_HMAP_HD uint64_t iter_bound(int64_t n, int64_t t) {
  return (uint64_t)t + 1 + (uint64_t)n * ((uint64_t)n + 1) / 2;
}

}  // namespace hmap
}  // namespace mp4x
