// All-gather, copy plans (broadcast / scatter / gather / ragged all-to-all) and the fused fp8
// two-shot over IPC-mapped peer buffers, plus the host runtime of the IPC mesh (allocation,
// handles, error words, spin bound).  Protocol: ipc_common.hpp.  The reducing families live in
// ipc_ar.hip (one-/two-shot), ipc_push.hip (zero-copy push) and ipc_rs.hip (reduce-scatter).
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdlib>

#include "ipc_common.hpp"
#include "../kernels/fp8.hpp"

namespace mp4x {

__global__ void k_ipc_bump_epoch(uint32_t* epoch_dev) {
  *epoch_dev = next_epoch(*epoch_dev);      // (wraps to 2: consecutive epochs alternate parity)
}

// ---------------------------------------------------------------- direct all-gather
// The second half of the two-shot as a collective of its own over RAGGED per-rank ranges
// (allgatherArray froms-tos): rank r pulls every peer's segment, the same offset from all p-1
// peers per step, so all links stream at once.
template <int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_gather(IpcPtrs P, Signal* self, int rank, Segs S,
                                                             int64_t maxlen, u32x4* __restrict__ out, uint32_t epoch,
                                                             const uint32_t* epoch_dev) {
  constexpr int p = NR;
  MP4X_DASSERT(rank >= 0 && rank < NR);
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int64_t stride = (int64_t)gridDim.x * kIpcThreads;
  for (int64_t v = (int64_t)blockIdx.x * kIpcThreads + threadIdx.x; v < maxlen; v += stride) {
    u32x4 x[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k)
      if (k != rank && S.lo[k] + v < S.hi[k]) x[k] = reinterpret_cast<const u32x4*>(P.data[k])[S.lo[k] + v];
#pragma unroll
    for (int k = 0; k < NR; ++k)
      if (k != rank && S.lo[k] + v < S.hi[k]) out[S.lo[k] + v] = x[k];
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// ---------------------------------------------------------------- copy plans (bcast / scatter / gather)
// The data-movement collectives as ONE kernel per call: a plan of up to kIpcMaxRanks "stage"
// items (this rank's input -> its own buffer, fused copy-in) and up to kPlanMaxPulls "pull" items
// (a peer's buffer -> this rank's output, over xGMI, all pulls interleaved so every link
// streams; two per peer: the sparse exchanges pull a row block and a key block from each).  Every item is walked with the same grid-stride relative index on every rank, so
// the vectors block b stages are exactly the vectors block b of the peers pull: per-block
// barriers suffice, as in the two-shot.  Units: 16-byte vectors.
struct CopyItem {
  int64_t src_off, dst_off, len;
  int64_t peer;          // pull: source rank; stage: unused
};
constexpr int kPlanMaxPulls = 2 * kIpcMaxRanks;
struct CopyPlan {
  CopyItem stage[kIpcMaxRanks];
  CopyItem pull[kPlanMaxPulls];
  int nstage, npull;
};

// NP: the pulls the kernel keeps in flight per vector step (kIpcMaxRanks, or kPlanMaxPulls for
// plans with more pulls than that: the wider form takes ~30 more VGPRs, so it only runs when needed).
template <int NP>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_copy_plan(IpcPtrs P, Signal* self, int rank, int p,
                                                                CopyPlan plan, const u32x4* __restrict__ src,
                                                                u32x4* __restrict__ out, uint32_t epoch,
                                                                const uint32_t* epoch_dev) {
  epoch = resolve_epoch(epoch, epoch_dev);
  const int64_t stride = (int64_t)gridDim.x * kIpcThreads;
  const int64_t off0 = (int64_t)blockIdx.x * kIpcThreads + threadIdx.x;
  u32x4* mine = reinterpret_cast<u32x4*>(const_cast<void*>(P.data[rank]));
  for (int i = 0; i < plan.nstage; ++i) {
    const CopyItem it = plan.stage[i];
    MP4X_DASSERT(it.len >= 0);
    for (int64_t v = off0; v < it.len; v += stride) mine[it.dst_off + v] = src[it.src_off + v];
  }
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  int64_t maxlen = 0;
  for (int i = 0; i < plan.npull; ++i) maxlen = plan.pull[i].len > maxlen ? plan.pull[i].len : maxlen;
  for (int64_t v = off0; v < maxlen; v += stride) {
    u32x4 x[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i)                     // every pull's vector in flight at once
      if (i < plan.npull && v < plan.pull[i].len)
        x[i] = reinterpret_cast<const u32x4*>(P.data[plan.pull[i].peer])[plan.pull[i].src_off + v];
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (i < plan.npull && v < plan.pull[i].len) out[plan.pull[i].dst_off + v] = x[i];
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// ---------------------------------------------------------------- fused fp8 two-shot (K6 on xGMI)
// Compressed allreduce with the block-scaled e4m3 codec on the links, in ONE kernel per piece
// (the quantise of this rank's input into its own IPC buffer runs just before, stream-ordered):
//   RS: for every 256-element quant block of chunk `rank`, each wave pulls the block's 256 fp8
//       bytes + scale from ALL p buffers at once (every xGMI link busy), dequantises and sums in
//       f32 registers, re-quantises (wave amax -> scale) into its OWN buffer, and writes the
//       dequantised result of that re-quantised block to `out` (so this rank's chunk holds
//       exactly what the peers will decode);
//   AG: every wave pulls the same block offset of every peer's chunk at once, dequantises
//       straight into `out`.
// Versus the RCCL form (all-to-all + fused dequant-reduce-requant + all-gather + dequant) no
// landing buffers are written and read back, and p-1 scale messages disappear.  Layout of the
// buffers: q bytes [0, M) then f32 scales at `soff` bytes, one per quant block; block j of chunk
// k is global quant block k * cb + j.  Block b of every rank visits the same chunk-relative j
// values in both phases, so the per-block barriers are the two-shot's.
// Wide form: every lane moves 16 bytes (16 e4m3 values) per peer per step, so one wave covers
// FOUR quant blocks (lanes 16g..16g+15 hold block g) and a block's amax is a 16-lane reduction;
// the four scales a wave needs sit in one 16-byte span, so the scale load is one request per
// wave.  Per element the arithmetic (rank-ordered FMAs, amax, e4m3 rounding) is the K6 codec's,
// so the result stays bit-identical to quantise -> dequant-reduce-requant -> dequantise.
__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));   // stays inside the 16-lane group
  return v;
}

// Output of one wave's 1024 dequantised values (4 consecutive quant blocks starting at
// global block b0): lane l holds values [16 l, 16 l + 16) — a 64-byte stride between lanes, so
// storing straight from registers would leave every store instruction 16 bytes per line.  The
// values go through a wave-private LDS tile (20-float lane pitch: 16-byte aligned, spread over
// the banks) and leave as 16-byte-per-lane CONTIGUOUS stores (1 KB of f32 per instruction).
// LO (the reduce-scatter half): only 4-element groups at or after element `lo` are stored, so a
// quant block shared with the previous rank's segment is written inside the own segment only.
constexpr int kFp8LdsPitch = 20;
template <int DT, bool LO = false>
__device__ __forceinline__ void fp8_wave_store(float* tile, const float (&y)[16], int lane, void* out,
                                               int64_t b0, int64_t cb_end, int64_t n, int64_t lo = 0) {
#pragma unroll
  for (int d = 0; d < 4; ++d)
    *reinterpret_cast<float4*>(tile + lane * kFp8LdsPitch + d * 4) = make_float4(y[4 * d], y[4 * d + 1],
                                                                                  y[4 * d + 2], y[4 * d + 3]);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's LDS writes are done
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int e = (d * 64 + lane) * 4;                  // value index inside the wave's 1024
    const float4 v = *reinterpret_cast<const float4*>(tile + (e >> 4) * kFp8LdsPitch + (e & 15));
    const int64_t blk = b0 + (e >> 8);
    bool in = blk < cb_end;
    if constexpr (LO) in = in && b0 * kQBlock + e >= lo;
    if (in) {
      float x[4] = {v.x, v.y, v.z, v.w};
      store4<DT>(out, b0 * kQBlock + e, n, x);
    }
  }
  __builtin_amdgcn_wave_barrier();      // the tile is rewritten by this wave's next step
}

template <int DT, int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_fp8_twoshot(IpcPtrs P, Signal* self, int rank, int64_t cb,
                                                                  int64_t soff, void* __restrict__ out, int64_t n,
                                                                  uint32_t epoch, const uint32_t* epoch_dev,
                                                                  float scale) {
  constexpr int p = NR;
  MP4X_DASSERT(rank >= 0 && rank < NR && blockIdx.x < kIpcMaxBlocks);
  __shared__ __attribute__((aligned(16))) float s_tile[kIpcThreads * kFp8LdsPitch];
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;                 // quant block of this lane within the wave's 4
  const int sub = lane & 15;               // 16-byte slot inside the 256-byte block
  constexpr int kWaves = kIpcThreads / 64;
  float* tile = s_tile + (threadIdx.x >> 6) * 64 * kFp8LdsPitch;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  const int64_t nquad = (cb + 3) / 4;      // wave steps per chunk
  {
    u32x4* myq = reinterpret_cast<u32x4*>(const_cast<void*>(P.data[rank]));
    float* mys = reinterpret_cast<float*>(reinterpret_cast<char*>(myq) + soff);
    for (int64_t t = w0; t < nquad; t += nw) {
      const int64_t j = t * 4 + g;                       // chunk-relative quant block
      const bool live = j < cb;
      const int64_t b = (int64_t)rank * cb + (live ? j : 0);   // global quant block
      u32x4 w[NR];
      float sc[NR];
#pragma unroll
      for (int k = 0; k < NR; ++k) {                      // every peer's 16 bytes in flight at once
        const u32x4* q = reinterpret_cast<const u32x4*>(P.data[k]);
        w[k] = live ? q[b * 16 + sub] : u32x4{0u, 0u, 0u, 0u};
        sc[k] = live ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b] : 0.0f;
      }
      float acc[4][4];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        acc[d][0] = acc[d][1] = acc[d][2] = acc[d][3] = 0.0f;
#pragma unroll
        for (int k = 0; k < NR; ++k) fp8_fma_acc(w[k][d], sc[k], acc[d]);   // rank order: deterministic
      }
      if (scale != 1.0f) {                                // fused average, before the re-quantisation
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[d][e] *= scale;
      }
      float m = 0.0f;
#pragma unroll
      for (int d = 0; d < 4; ++d)
        m = fmaxf(m, fmaxf(fmaxf(fabsf(acc[d][0]), fabsf(acc[d][1])), fmaxf(fabsf(acc[d][2]), fabsf(acc[d][3]))));
      m = group16_max(m);
      const float bscale = m > 0.0f ? m / kFp8Max : 1.0f;
      const float inv = 1.0f / bscale;
      u32x4 qq;
#pragma unroll
      for (int d = 0; d < 4; ++d) qq[d] = pack_fp8(acc[d], inv);
      if (live) {
        myq[b * 16 + sub] = qq;                           // read by the peers after the mid barrier
        if (sub == 0) mys[b] = bscale;
      }
      float y[16];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float yy[4];
        unpack_fp8(qq[d], bscale, yy);
        y[4 * d] = yy[0]; y[4 * d + 1] = yy[1]; y[4 * d + 2] = yy[2]; y[4 * d + 3] = yy[3];
      }
      fp8_wave_store<DT>(tile, y, lane, out, (int64_t)rank * cb + t * 4, (int64_t)rank * cb + cb, n);
    }
  }
  if (!block_barrier(P, 1, rank, p, epoch, self)) return;
  for (int64_t t = w0; t < nquad; t += nw) {
    const int64_t j = t * 4 + g;
    const bool live = j < cb;
    u32x4 w[NR];
    float sc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (k == rank) continue;
      const u32x4* q = reinterpret_cast<const u32x4*>(P.data[k]);
      const int64_t b = (int64_t)k * cb + (live ? j : 0);
      w[k] = live ? q[b * 16 + sub] : u32x4{0u, 0u, 0u, 0u};
      sc[k] = live ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (k == rank) continue;
      float y[16];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float yy[4];
        unpack_fp8(w[k][d], sc[k], yy);
        y[4 * d] = yy[0]; y[4 * d + 1] = yy[1]; y[4 * d + 2] = yy[2]; y[4 * d + 3] = yy[3];
      }
      fp8_wave_store<DT>(tile, y, lane, out, (int64_t)k * cb + t * 4, (int64_t)k * cb + cb, n);
    }
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// ---------------------------------------------------------------- the two halves as collectives
// reduceScatterArray / allgatherArray with the fp8 operand: the halves of the two-shot over RAGGED
// per-rank segments, each a kernel of its own with the wide layout above (16 bytes per lane per
// peer, four quant blocks per wave step, every peer's load issued before the first FMA, stores
// through the wave's LDS tile) and a start and an end barrier.  The quantise of this rank's data
// into its own buffer runs just before, stream-ordered, as in the allreduce.
//
// Reduce-scatter: every rank quantised the WHOLE range of the piece on one block grid counted
// from the piece's first element (q bytes at 0, f32 scales at `soff`, `nblk` blocks).  This rank
// reduces the blocks [blo, bhi) that touch its segment [elo, ehi) (elements from the piece start,
// multiples of 4), sums them in rank order in f32 and stores with ONE rounding, in place, only the
// 4-element groups inside its segment: a block that straddles two segments is reduced by both
// ranks and written by each inside its own.  Nothing is re-quantised.  Every rank launches the
// same grid (sized from the largest block count of any rank), also for an empty segment.
template <int DT, int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_fp8_rs(IpcPtrs P, Signal* self, int rank, int64_t blo,
                                                             int64_t bhi, int64_t nblk, int64_t soff,
                                                             void* __restrict__ out, int64_t elo, int64_t ehi,
                                                             uint32_t epoch, const uint32_t* epoch_dev) {
  constexpr int p = NR;
  MP4X_DASSERT(rank >= 0 && rank < NR && blockIdx.x < kIpcMaxBlocks);
  MP4X_DASSERT(blo >= 0 && blo <= bhi && bhi <= nblk && soff >= nblk * kQBlock);
  MP4X_DASSERT(elo <= ehi && (elo == ehi || (elo >= blo * kQBlock && ehi <= bhi * kQBlock)));
  (void)nblk;
  __shared__ __attribute__((aligned(16))) float s_tile[kIpcThreads * kFp8LdsPitch];
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;                 // quant block of this lane within the wave's 4
  const int sub = lane & 15;               // 16-byte slot inside the 256-byte block
  constexpr int kWaves = kIpcThreads / 64;
  float* tile = s_tile + (threadIdx.x >> 6) * 64 * kFp8LdsPitch;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  const int64_t nquad = (bhi - blo + 3) / 4;             // wave steps over the own blocks
  for (int64_t t = w0; t < nquad; t += nw) {
    const int64_t j = blo + t * 4 + g;                   // quant block on the piece's grid
    const bool live = j < bhi;
    const int64_t b = live ? j : blo;
    MP4X_DASSERT(b >= 0 && b < nblk);
    u32x4 w[NR];
    float sc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {                        // every peer's 16 bytes in flight at once
      const u32x4* q = reinterpret_cast<const u32x4*>(P.data[k]);
      w[k] = live ? q[b * 16 + sub] : u32x4{0u, 0u, 0u, 0u};
      sc[k] = live ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b] : 0.0f;
    }
    float y[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < NR; ++k) fp8_fma_acc(w[k][d], sc[k], acc);   // rank order: deterministic
      y[4 * d] = acc[0]; y[4 * d + 1] = acc[1]; y[4 * d + 2] = acc[2]; y[4 * d + 3] = acc[3];
    }
    fp8_wave_store<DT, true>(tile, y, lane, out, blo + t * 4, bhi, ehi, elo);
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// All-gather: rank k quantised ITS segment of the piece on a block grid counted from the segment's
// start; its buffer holds only that (q bytes at 0, scales at `soff`, which comes from the largest
// segment).  Every rank pulls the blocks of every segment — its own included, from its own
// buffer, so all ranks end up with the same bytes — and dequantises them straight into
// out[S.lo[k], S.hi[k]) (elements of the output; S.lo 16-byte aligned offsets).
template <int DT, int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_fp8_ag(IpcPtrs P, Signal* self, int rank, Segs S,
                                                             int64_t maxblk, int64_t soff, void* __restrict__ out,
                                                             uint32_t epoch, const uint32_t* epoch_dev) {
  constexpr int p = NR;
  using ST = typename Elem<DT>::S;
  MP4X_DASSERT(rank >= 0 && rank < NR && blockIdx.x < kIpcMaxBlocks);
  MP4X_DASSERT(maxblk >= 0 && soff >= maxblk * kQBlock);
  __shared__ __attribute__((aligned(16))) float s_tile[kIpcThreads * kFp8LdsPitch];
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int sub = lane & 15;
  constexpr int kWaves = kIpcThreads / 64;
  float* tile = s_tile + (threadIdx.x >> 6) * 64 * kFp8LdsPitch;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  const int64_t nquad = (maxblk + 3) / 4;                // wave steps over the largest segment
  int64_t nb[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    MP4X_DASSERT(S.lo[k] >= 0 && S.lo[k] <= S.hi[k]);
    nb[k] = (S.hi[k] - S.lo[k] + kQBlock - 1) / kQBlock;  // quant blocks of segment k
    MP4X_DASSERT(nb[k] <= maxblk);
  }
  for (int64_t t = w0; t < nquad; t += nw) {
    const int64_t j = t * 4 + g;                         // segment-relative quant block
    u32x4 w[NR];
    float sc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {                        // every peer's 16 bytes in flight at once
      const u32x4* q = reinterpret_cast<const u32x4*>(P.data[k]);
      const bool live = j < nb[k];
      const int64_t b = live ? j : 0;
      w[k] = live ? q[b * 16 + sub] : u32x4{0u, 0u, 0u, 0u};
      sc[k] = live ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (t * 4 >= nb[k]) continue;                       // wave-uniform: segment k ends before this step
      float y[16];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        // the codec's one-input dequant-reduce, fma(code, scale, +0): what the reduce-scatter half
        // gives for p = 1 (a -0 code decodes to +0, where unpack_fp8's product would keep the sign)
        float yy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        fp8_fma_acc(w[k][d], sc[k], yy);
        y[4 * d] = yy[0]; y[4 * d + 1] = yy[1]; y[4 * d + 2] = yy[2]; y[4 * d + 3] = yy[3];
      }
      fp8_wave_store<DT>(tile, y, lane, reinterpret_cast<ST*>(out) + S.lo[k], t * 4, nb[k], S.hi[k] - S.lo[k]);
    }
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// Ragged all-to-all: rank k quantised its WHOLE send buffer (rows grouped by destination,
// flattened) on ONE block grid counted from the buffer's first element (q bytes at 0, scales at
// `soff`, which comes from the largest send of any rank).  This rank pulls from every peer k the
// quant blocks that touch k's segment for it, [S.elo[k], S.ehi[k]) of k's buffer, and dequantises
// them to out[S.dst[k] ...] with one rounding; a block that straddles two destinations is decoded
// by both receivers and stored by each inside its own segment only (the reduce-scatter's LO
// store at the front, the element bound at the back).  Every rank launches the same grid (sized
// by the caller from the largest segment anywhere in the count matrix), also when it receives
// nothing; the wave steps are this rank's own, the barriers are per block.
template <int DT, int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_fp8_a2a(IpcPtrs P, Signal* self, int rank, A2aSegs S,
                                                              int64_t soff, void* __restrict__ out,
                                                              uint32_t epoch, const uint32_t* epoch_dev) {
  constexpr int p = NR;
  using ST = typename Elem<DT>::S;
  MP4X_DASSERT(rank >= 0 && rank < NR && blockIdx.x < kIpcMaxBlocks);
  MP4X_DASSERT(soff >= 0 && (soff & 15) == 0);
  __shared__ __attribute__((aligned(16))) float s_tile[kIpcThreads * kFp8LdsPitch];
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int sub = lane & 15;
  constexpr int kWaves = kIpcThreads / 64;
  float* tile = s_tile + (threadIdx.x >> 6) * 64 * kFp8LdsPitch;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  int64_t cb0[NR], cbe[NR];                              // quant blocks of peer k's grid that touch its segment
  int64_t nquad = 0;                                     // wave steps over the largest of them
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    MP4X_DASSERT(S.elo[k] >= 0 && S.elo[k] <= S.ehi[k] && S.dst[k] >= 0);
    MP4X_DASSERT(((S.elo[k] | S.ehi[k] | S.dst[k]) & 3) == 0);
    cb0[k] = S.elo[k] / kQBlock;
    cbe[k] = S.ehi[k] > S.elo[k] ? (S.ehi[k] + kQBlock - 1) / kQBlock : cb0[k];
    MP4X_DASSERT(soff >= cbe[k] * kQBlock);
    const int64_t q4 = (cbe[k] - cb0[k] + 3) / 4;
    nquad = q4 > nquad ? q4 : nquad;
  }
  for (int64_t t = w0; t < nquad; t += nw) {
    u32x4 w[NR];
    float sc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {                        // every peer's 16 bytes in flight at once
      const u32x4* q = reinterpret_cast<const u32x4*>(P.data[k]);
      const int64_t j = cb0[k] + t * 4 + g;               // quant block on peer k's grid
      const bool live = j < cbe[k];
      const int64_t b = live ? j : cb0[k];
      MP4X_DASSERT(b >= 0 && (!live || (b + 1) * kQBlock <= soff));
      w[k] = live ? q[b * 16 + sub] : u32x4{0u, 0u, 0u, 0u};
      sc[k] = live ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (cb0[k] + t * 4 >= cbe[k]) continue;             // wave-uniform: segment k ends before this step
      float y[16];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        // the codec's one-input dequant-reduce, fma(code, scale, +0), as in the all-gather
        float yy[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        fp8_fma_acc(w[k][d], sc[k], yy);
        y[4 * d] = yy[0]; y[4 * d + 1] = yy[1]; y[4 * d + 2] = yy[2]; y[4 * d + 3] = yy[3];
      }
      // element e of peer k's buffer lands at out[dst[k] + e - elo[k]]
      fp8_wave_store<DT, true>(tile, y, lane, reinterpret_cast<ST*>(out) + (S.dst[k] - S.elo[k]), cb0[k] + t * 4,
                               cbe[k], S.ehi[k], S.elo[k]);
    }
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

// The r1 form (4 bytes per lane per peer, one wave per quant block), kept for A/B measurement
// (MP4X_FP8_NARROW=1); bit-identical results.
template <int DT, int NR>
__global__ __launch_bounds__(kIpcThreads) void k_ipc_fp8_twoshot_narrow(IpcPtrs P, Signal* self, int rank, int64_t cb,
                                                                  int64_t soff, void* __restrict__ out, int64_t n,
                                                                  uint32_t epoch, const uint32_t* epoch_dev,
                                                                  float scale) {
  constexpr int p = NR;
  MP4X_DASSERT(rank >= 0 && rank < NR && blockIdx.x < kIpcMaxBlocks);
  epoch = resolve_epoch(epoch, epoch_dev);
  if (!block_barrier(P, 0, rank, p, epoch, self)) return;
  const int lane = threadIdx.x & 63;
  constexpr int kWaves = kIpcThreads / 64;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * kWaves;
  {
    uint32_t* myq = reinterpret_cast<uint32_t*>(const_cast<void*>(P.data[rank]));
    float* mys = reinterpret_cast<float*>(reinterpret_cast<char*>(myq) + soff);
    for (int64_t j = w0; j < cb; j += nw) {
      const int64_t b = (int64_t)rank * cb + j;          // global quant block
      uint32_t w[NR];
      float sc[NR];
#pragma unroll
      for (int k = 0; k < NR; ++k) {                      // every peer's block in flight at once
        const uint32_t* q = reinterpret_cast<const uint32_t*>(P.data[k]);
        w[k] = q[b * 64 + lane];
        sc[k] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b];
      }
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < NR; ++k) fp8_fma_acc(w[k], sc[k], acc);   // rank order: deterministic
      if (scale != 1.0f) {                                // fused average, before the re-quantisation
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] *= scale;
      }
      float m = fmaxf(fmaxf(fabsf(acc[0]), fabsf(acc[1])), fmaxf(fabsf(acc[2]), fabsf(acc[3])));
      m = wave_max(m);
      const float bscale = m > 0.0f ? m / kFp8Max : 1.0f;
      const uint32_t qq = pack_fp8(acc, 1.0f / bscale);
      myq[b * 64 + lane] = qq;                            // read by the peers after the mid barrier
      if (lane == 0) mys[b] = bscale;
      float y[4];
      unpack_fp8(qq, bscale, y);
      store4<DT>(out, b * kQBlock + lane * 4, n, y);
    }
  }
  if (!block_barrier(P, 1, rank, p, epoch, self)) return;
  for (int64_t j = w0; j < cb; j += nw) {
    uint32_t w[NR];
    float sc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (k == rank) continue;
      const uint32_t* q = reinterpret_cast<const uint32_t*>(P.data[k]);
      const int64_t b = (int64_t)k * cb + j;
      w[k] = q[b * 64 + lane];
      sc[k] = reinterpret_cast<const float*>(reinterpret_cast<const char*>(q) + soff)[b];
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      if (k == rank) continue;
      const int64_t b = (int64_t)k * cb + j;
      if (b * kQBlock >= n) continue;
      float y[4];
      unpack_fp8(w[k], sc[k], y);
      store4<DT>(out, b * kQBlock + lane * 4, n, y);
    }
  }
  block_barrier(P, 2, rank, p, epoch, self);
}

template <int DT>
static int fp8_nr(const IpcPtrs& P, Signal* self, int rank, int p, int64_t cb, int64_t soff, void* out, int64_t n,
                  uint32_t epoch, const uint32_t* edev, float scale, int blocks, hipStream_t st, bool narrow) {
#define MP4X_FP8_CASE(N)                                                                                     \
  case N:                                                                                                    \
    if (narrow)                                                                                              \
      hipLaunchKernelGGL((k_ipc_fp8_twoshot_narrow<DT, N>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self,   \
                         rank, cb, soff, out, n, epoch, edev, scale);                                        \
    else                                                                                                     \
      hipLaunchKernelGGL((k_ipc_fp8_twoshot<DT, N>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self, rank,   \
                         cb, soff, out, n, epoch, edev, scale);                                              \
    return (int)hipGetLastError();
  switch (p) {
    MP4X_FP8_CASE(2) MP4X_FP8_CASE(3) MP4X_FP8_CASE(4) MP4X_FP8_CASE(5) MP4X_FP8_CASE(6) MP4X_FP8_CASE(7)
    MP4X_FP8_CASE(8)
    default: return MP4X_E_BADARG;
  }
#undef MP4X_FP8_CASE
}

}  // namespace mp4x

using namespace mp4x;

extern "C" size_t mp4x_ipc_signal_bytes(void) { return sizeof(Signal); }

extern "C" int mp4x_ipc_alloc(size_t bytes, void** ptr) {
  hipError_t e = hipExtMallocWithFlags(ptr, bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) return (int)e;
  e = hipMemset(*ptr, 0, bytes);
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

extern "C" int mp4x_ipc_free(void* ptr) { return (int)hipFree(ptr); }

extern "C" int mp4x_ipc_alloc_data(size_t bytes, int coarse, void** ptr) {
  if (!coarse) return mp4x_ipc_alloc(bytes, ptr);
  hipError_t e = hipMalloc(ptr, bytes);
  if (e != hipSuccess) return (int)e;
  e = hipMemset(*ptr, 0, bytes);
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceSynchronize();
}

extern "C" int mp4x_dev_alloc(size_t bytes, void** ptr) { return (int)hipMalloc(ptr, bytes); }

extern "C" int mp4x_host_word_alloc(void** host_ptr, void** dev_ptr) {
  hipError_t e = hipHostMalloc(host_ptr, 64, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return (int)e;
  __builtin_memset(*host_ptr, 0, 64);
  return (int)hipHostGetDevicePointer(dev_ptr, *host_ptr, 0);
}

extern "C" int mp4x_host_word_free(void* host_ptr) { return (int)hipHostFree(host_ptr); }

extern "C" int mp4x_ipc_set_host_error(void* signal, void* dev_word) {
  const uint64_t v = (uint64_t)(uintptr_t)dev_word;
  hipError_t e = hipMemcpy((char*)signal + offsetof(Signal, host_err), &v, sizeof(v), hipMemcpyHostToDevice);
  return (int)e;
}

extern "C" int mp4x_ipc_set_spin(void* signal, double seconds, void* stream) {
  if (!(seconds > 0.0) || !signal) return MP4X_E_BADARG;
  const uint64_t ticks = (uint64_t)(seconds * 1.0e8);   // the stream is synchronised below
  char* w = (char*)signal + offsetof(Signal, spin_ticks);
  hipError_t e = hipMemcpyAsync(w, &ticks, sizeof(ticks), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  return (int)hipStreamSynchronize((hipStream_t)stream);
}

extern "C" int mp4x_ipc_bump_epoch(uint32_t* epoch_dev, void* stream) {
  hipLaunchKernelGGL(k_ipc_bump_epoch, dim3(1), dim3(1), 0, (hipStream_t)stream, epoch_dev);
  return (int)hipGetLastError();
}

extern "C" int mp4x_device_pci_id(char* buf, int len) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  return (int)hipDeviceGetPCIBusId(buf, len, dev);
}

extern "C" int mp4x_ipc_handle_size(void) { return (int)sizeof(hipIpcMemHandle_t); }

extern "C" int mp4x_mem_range(void* ptr, void** base, size_t* size) {
  hipDeviceptr_t b = nullptr;
  size_t sz = 0;
  hipError_t e = hipMemGetAddressRange(&b, &sz, (hipDeviceptr_t)ptr);
  *base = (void*)b;
  *size = sz;
  return (int)e;
}

extern "C" int mp4x_ipc_get_handle(void* ptr, void* handle_out) {
  return (int)hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(handle_out), ptr);
}

extern "C" int mp4x_ipc_open_handle(const void* handle, void** ptr) {
  hipIpcMemHandle_t h;
  __builtin_memcpy(&h, handle, sizeof(h));
  return (int)hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess);
}

extern "C" int mp4x_ipc_close_handle(void* ptr) { return (int)hipIpcCloseMemHandle(ptr); }

extern "C" int mp4x_memcpy_async(void* dst, const void* src, size_t bytes, void* stream) {
  return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

extern "C" int mp4x_ipc_error_word(void* signal, uint32_t* err, int clear, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)signal + offsetof(Signal, error);
  hipError_t e = hipMemcpyAsync(err, w, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && clear) e = hipMemsetAsync(w, 0, 4, st);
  if (e != hipSuccess) return (int)e;
  return (int)hipStreamSynchronize(st);
}

extern "C" int mp4x_ipc_allgather(void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                  const int64_t* seg_lo, const int64_t* seg_hi, void* out, uint32_t epoch, int blocks,
                                  const uint32_t* epoch_dev, void* stream) {
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  if ((uintptr_t)out & 15) return MP4X_E_BADARG;
  Segs S;
  int64_t maxlen = 0;
  for (int k = 0; k < kIpcMaxRanks; ++k) {
    S.lo[k] = k < p ? seg_lo[k] : 0;
    S.hi[k] = k < p ? seg_hi[k] : 0;
    if (k < p && (S.lo[k] < 0 || S.hi[k] < S.lo[k])) return MP4X_E_BADARG;
    if (S.hi[k] - S.lo[k] > maxlen) maxlen = S.hi[k] - S.lo[k];
  }
  blocks = ipc_blocks(blocks, maxlen);
  Signal* self = (Signal*)signal_ptrs[rank];
  hipStream_t st = (hipStream_t)stream;
#define MP4X_AG_CASE(N)                                                                                     \
  case N:                                                                                                   \
    hipLaunchKernelGGL((k_ipc_gather<N>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self, rank, S, maxlen, \
                       (u32x4*)out, epoch, epoch_dev);                                                      \
    return (int)hipGetLastError();
  switch (p) {
    MP4X_AG_CASE(2) MP4X_AG_CASE(3) MP4X_AG_CASE(4) MP4X_AG_CASE(5) MP4X_AG_CASE(6) MP4X_AG_CASE(7) MP4X_AG_CASE(8)
    default: return MP4X_E_BADARG;
  }
#undef MP4X_AG_CASE
}

extern "C" int mp4x_ipc_fp8_allreduce(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                      int64_t cb, int64_t soff, void* out, int64_t n, uint32_t epoch, int blocks,
                                      const uint32_t* epoch_dev, float scale, void* stream) {
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  if (cb <= 0 || n <= 0 || n > (int64_t)p * cb * kQBlock || (soff & 15) || ((uintptr_t)out & 15))
    return MP4X_E_BADARG;
  if (soff < (int64_t)p * cb * kQBlock) return MP4X_E_BADARG;     // scales after the q bytes
  static const bool narrow = getenv("MP4X_FP8_NARROW") && getenv("MP4X_FP8_NARROW")[0] == '1';
  if (blocks <= 0) {
    const int64_t waves = narrow ? cb : (cb + 3) / 4;               // one wave per 4 quant blocks
    int64_t b = (waves + kIpcThreads / 64 - 1) / (kIpcThreads / 64);
    blocks = (int)(b < 1 ? 1 : (b > kIpcMaxBlocks ? kIpcMaxBlocks : b));
  }
  if (blocks > kIpcMaxBlocks) blocks = kIpcMaxBlocks;
  Signal* self = (Signal*)signal_ptrs[rank];
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case MP4X_F32: return fp8_nr<MP4X_F32>(P, self, rank, p, cb, soff, out, n, epoch, epoch_dev, scale, blocks, st, narrow);
    case MP4X_BF16: return fp8_nr<MP4X_BF16>(P, self, rank, p, cb, soff, out, n, epoch, epoch_dev, scale, blocks, st, narrow);
    case MP4X_F16: return fp8_nr<MP4X_F16>(P, self, rank, p, cb, soff, out, n, epoch, epoch_dev, scale, blocks, st, narrow);
    default: return MP4X_E_UNSUPPORTED;
  }
}

// Grid of the fp8 halves when the caller passes none: one wave per 4 quant blocks of the LARGEST
// share of any rank (rank-independent), 8 waves per block.
static int fp8_half_blocks(int blocks, int64_t maxblk) {
  if (blocks <= 0) {
    const int64_t waves = (maxblk + 3) / 4;
    const int64_t b = (waves + kIpcThreads / 64 - 1) / (kIpcThreads / 64);
    blocks = (int)(b < 1 ? 1 : b);
  }
  return blocks > kIpcMaxBlocks ? kIpcMaxBlocks : blocks;
}

static int fp8_half_common_check(int dtype, int rank, int p, int64_t nblk, int64_t soff, const int64_t* seg_lo,
                                 const int64_t* seg_hi, const void* out) {
  if (dtype != MP4X_F32 && dtype != MP4X_BF16 && dtype != MP4X_F16) return MP4X_E_UNSUPPORTED;
  if (p < 2 || p > kIpcMaxRanks || rank < 0 || rank >= p) return MP4X_E_BADARG;
  if (nblk <= 0 || (soff & 15) || soff < nblk * kQBlock) return MP4X_E_BADARG;     // scales after the q bytes
  if (!out || ((uintptr_t)out & 15) || !seg_lo || !seg_hi) return MP4X_E_BADARG;
  return 0;
}

// The block range [*blo, *bhi) of segment [lo, hi) on a 256-element grid (empty for an empty segment).
static void fp8_seg_blocks(int64_t lo, int64_t hi, int64_t* blo, int64_t* bhi) {
  *blo = lo / kQBlock;
  *bhi = hi > lo ? (hi + kQBlock - 1) / kQBlock : *blo;
}

extern "C" int mp4x_ipc_fp8_reduce_scatter_check(int dtype, int rank, int p, int64_t nblk, int64_t soff,
                                                 const int64_t* seg_lo, const int64_t* seg_hi, const void* out) {
  if (int e = fp8_half_common_check(dtype, rank, p, nblk, soff, seg_lo, seg_hi, out)) return e;
  int64_t prev = 0;
  for (int k = 0; k < p; ++k) {        // ascending, inside the quantised blocks, whole 4-element groups
    if (seg_lo[k] < prev || seg_hi[k] < seg_lo[k] || seg_hi[k] > nblk * kQBlock) return MP4X_E_BADARG;
    if ((seg_lo[k] | seg_hi[k]) & 3) return MP4X_E_BADARG;
    prev = seg_hi[k];
  }
  return 0;
}

extern "C" int mp4x_ipc_fp8_reduce_scatter(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank,
                                           int p, int64_t nblk, int64_t soff, const int64_t* seg_lo,
                                           const int64_t* seg_hi, void* out, uint32_t epoch, int blocks,
                                           const uint32_t* epoch_dev, void* stream) {
  if (int e = mp4x_ipc_fp8_reduce_scatter_check(dtype, rank, p, nblk, soff, seg_lo, seg_hi, out)) return e;
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  int64_t maxblk = 0, blo = 0, bhi = 0;
  for (int k = 0; k < p; ++k) {
    int64_t a, b;
    fp8_seg_blocks(seg_lo[k], seg_hi[k], &a, &b);
    if (b - a > maxblk) maxblk = b - a;
    if (k == rank) { blo = a; bhi = b; }
  }
  blocks = fp8_half_blocks(blocks, maxblk);
  const int64_t elo = seg_lo[rank], ehi = seg_hi[rank];
  Signal* self = (Signal*)signal_ptrs[rank];
  hipStream_t st = (hipStream_t)stream;
  return with_nr(p, [&](auto nrc) {
    constexpr int NR = decltype(nrc)::value;
#define MP4X_FP8RS_CASE(DT)                                                                                    \
  case DT:                                                                                                     \
    hipLaunchKernelGGL((k_ipc_fp8_rs<DT, NR>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self, rank, blo, bhi, \
                       nblk, soff, out, elo, ehi, epoch, epoch_dev);                                           \
    return (int)hipGetLastError();
    switch (dtype) {
      MP4X_FP8RS_CASE(MP4X_F32) MP4X_FP8RS_CASE(MP4X_BF16) MP4X_FP8RS_CASE(MP4X_F16)
      default: return (int)MP4X_E_UNSUPPORTED;
    }
#undef MP4X_FP8RS_CASE
  });
}

extern "C" int mp4x_ipc_fp8_allgather_check(int dtype, int rank, int p, int64_t maxblk, int64_t soff,
                                            const int64_t* seg_lo, const int64_t* seg_hi, const void* out) {
  if (int e = fp8_half_common_check(dtype, rank, p, maxblk, soff, seg_lo, seg_hi, out)) return e;
  for (int k = 0; k < p; ++k) {        // not descending, no longer than the quantised blocks, 4-element groups
    if (seg_lo[k] < 0 || seg_hi[k] < seg_lo[k] || seg_hi[k] - seg_lo[k] > maxblk * kQBlock) return MP4X_E_BADARG;
    if ((seg_lo[k] | seg_hi[k]) & 3) return MP4X_E_BADARG;
  }
  return 0;
}

extern "C" int mp4x_ipc_fp8_allgather(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                      int64_t maxblk, int64_t soff, const int64_t* seg_lo, const int64_t* seg_hi,
                                      void* out, uint32_t epoch, int blocks, const uint32_t* epoch_dev,
                                      void* stream) {
  if (int e = mp4x_ipc_fp8_allgather_check(dtype, rank, p, maxblk, soff, seg_lo, seg_hi, out)) return e;
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  Segs S;
  int64_t used = 0;
  for (int k = 0; k < kIpcMaxRanks; ++k) {
    S.lo[k] = k < p ? seg_lo[k] : 0;
    S.hi[k] = k < p ? seg_hi[k] : 0;
    const int64_t nb = (S.hi[k] - S.lo[k] + kQBlock - 1) / kQBlock;
    if (nb > used) used = nb;
  }
  blocks = fp8_half_blocks(blocks, used);
  Signal* self = (Signal*)signal_ptrs[rank];
  hipStream_t st = (hipStream_t)stream;
  return with_nr(p, [&](auto nrc) {
    constexpr int NR = decltype(nrc)::value;
#define MP4X_FP8AG_CASE(DT)                                                                                   \
  case DT:                                                                                                    \
    hipLaunchKernelGGL((k_ipc_fp8_ag<DT, NR>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self, rank, S, used, \
                       soff, out, epoch, epoch_dev);                                                          \
    return (int)hipGetLastError();
    switch (dtype) {
      MP4X_FP8AG_CASE(MP4X_F32) MP4X_FP8AG_CASE(MP4X_BF16) MP4X_FP8AG_CASE(MP4X_F16)
      default: return (int)MP4X_E_UNSUPPORTED;
    }
#undef MP4X_FP8AG_CASE
  });
}

extern "C" int mp4x_ipc_fp8_alltoall_check(int dtype, int rank, int p, int64_t soff, const int64_t* elo,
                                           const int64_t* ehi, const int64_t* dst, const int64_t* nblk_peer,
                                           const void* out) {
  if (dtype != MP4X_F32 && dtype != MP4X_BF16 && dtype != MP4X_F16) return MP4X_E_UNSUPPORTED;
  if (p < 2 || p > kIpcMaxRanks || rank < 0 || rank >= p) return MP4X_E_BADARG;
  if (!elo || !ehi || !dst || !nblk_peer || ((uintptr_t)out & 15)) return MP4X_E_BADARG;
  int64_t maxblk = 0, end = 0;
  for (int k = 0; k < p; ++k) {
    if (nblk_peer[k] < 0) return MP4X_E_BADARG;
    if (nblk_peer[k] > maxblk) maxblk = nblk_peer[k];
  }
  if (soff < 0 || (soff & 15) || soff < maxblk * kQBlock) return MP4X_E_BADARG;    // scales after the q bytes
  for (int k = 0; k < p; ++k) {
    // not descending, inside peer k's quantised blocks, whole 4-element groups on both sides
    if (elo[k] < 0 || ehi[k] < elo[k] || ehi[k] > nblk_peer[k] * kQBlock) return MP4X_E_BADARG;
    if ((elo[k] | ehi[k] | dst[k]) & 3) return MP4X_E_BADARG;
    if ((dst[k] - elo[k]) & 3) return MP4X_E_BADARG;     // store4's vector path stays aligned
    if (dst[k] < end) return MP4X_E_BADARG;              // source-rank order, no overlap in `out`
    end = dst[k] + (ehi[k] - elo[k]);
    if (ehi[k] > elo[k] && !out) return MP4X_E_BADARG;
  }
  return 0;
}

extern "C" int mp4x_ipc_fp8_alltoall(int dtype, void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                     int64_t soff, const int64_t* elo, const int64_t* ehi, const int64_t* dst,
                                     const int64_t* nblk_peer, void* out, uint32_t epoch, int blocks,
                                     const uint32_t* epoch_dev, void* stream) {
  if (int e = mp4x_ipc_fp8_alltoall_check(dtype, rank, p, soff, elo, ehi, dst, nblk_peer, out)) return e;
  // this rank sees its own column of the count matrix only: the grid, which must be the same on
  // every rank (per-block barriers), is the caller's
  if (blocks < 1) return MP4X_E_BADARG;
  if (blocks > kIpcMaxBlocks) blocks = kIpcMaxBlocks;
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  A2aSegs S;
  for (int k = 0; k < kIpcMaxRanks; ++k) {
    S.elo[k] = k < p ? elo[k] : 0;
    S.ehi[k] = k < p ? ehi[k] : 0;
    S.dst[k] = k < p ? dst[k] : 0;
  }
  Signal* self = (Signal*)signal_ptrs[rank];
  hipStream_t st = (hipStream_t)stream;
  return with_nr(p, [&](auto nrc) {
    constexpr int NR = decltype(nrc)::value;
#define MP4X_FP8A2A_CASE(DT)                                                                                   \
  case DT:                                                                                                     \
    hipLaunchKernelGGL((k_ipc_fp8_a2a<DT, NR>), dim3(blocks), dim3(kIpcThreads), 0, st, P, self, rank, S, soff, \
                       out, epoch, epoch_dev);                                                                 \
    return (int)hipGetLastError();
    switch (dtype) {
      MP4X_FP8A2A_CASE(MP4X_F32) MP4X_FP8A2A_CASE(MP4X_BF16) MP4X_FP8A2A_CASE(MP4X_F16)
      default: return (int)MP4X_E_UNSUPPORTED;
    }
#undef MP4X_FP8A2A_CASE
  });
}

extern "C" int mp4x_memset_async(void* dst, int value, size_t bytes, void* stream) {
  return (int)hipMemsetAsync(dst, value, bytes, (hipStream_t)stream);
}

extern "C" int mp4x_ipc_copy_plan_check(int rank, int p, const int64_t* stage, int nstage, const int64_t* pull,
                                        int npull, const void* src, const void* out, int64_t buf_vecs) {
  if (p < 2 || p > kIpcMaxRanks || rank < 0 || rank >= p) return MP4X_E_BADARG;
  if (nstage < 0 || nstage > kIpcMaxRanks || npull < 0 || npull > kPlanMaxPulls) return MP4X_E_BADARG;
  if ((nstage && (!src || ((uintptr_t)src & 15))) || (npull && (!out || ((uintptr_t)out & 15)))) return MP4X_E_BADARG;
  for (int i = 0; i < nstage; ++i) {
    const int64_t* it = stage + 4 * i;                    // {src_off, dst_off, len, -}
    if (it[2] < 0 || it[1] < 0 || it[1] + it[2] > buf_vecs) return MP4X_E_BADARG;   // inside the own buffer
  }
  for (int i = 0; i < npull; ++i) {
    const int64_t* it = pull + 4 * i;                     // {src_off, dst_off, len, peer}
    if (it[2] < 0 || it[3] < 0 || it[3] >= p || it[0] < 0 || it[0] + it[2] > buf_vecs)
      return MP4X_E_BADARG;                               // pulls stay inside the peer's buffer
  }
  return 0;
}

extern "C" int mp4x_ipc_copy_plan(void* const* data_ptrs, void* const* signal_ptrs, int rank, int p,
                                  const int64_t* stage, int nstage, const int64_t* pull, int npull, const void* src,
                                  void* out, int64_t grid_len, int64_t buf_vecs, uint32_t epoch, int blocks,
                                  const uint32_t* epoch_dev, void* stream) {
  if (int e = mp4x_ipc_copy_plan_check(rank, p, stage, nstage, pull, npull, src, out, buf_vecs)) return e;
  IpcPtrs P;
  if (int e = ipc_prepare(data_ptrs, signal_ptrs, rank, p, &P)) return e;
  CopyPlan plan;
  plan.nstage = nstage;
  plan.npull = npull;
  for (int i = 0; i < kIpcMaxRanks; ++i)
    plan.stage[i] = i < nstage ? CopyItem{stage[4 * i], stage[4 * i + 1], stage[4 * i + 2], 0} : CopyItem{0, 0, 0, 0};
  for (int i = 0; i < kPlanMaxPulls; ++i)
    plan.pull[i] = i < npull ? CopyItem{pull[4 * i], pull[4 * i + 1], pull[4 * i + 2], pull[4 * i + 3]}
                             : CopyItem{0, 0, 0, 0};
  blocks = ipc_blocks(blocks, grid_len);
  if (npull <= kIpcMaxRanks)
    hipLaunchKernelGGL(k_ipc_copy_plan<kIpcMaxRanks>, dim3(blocks), dim3(kIpcThreads), 0, (hipStream_t)stream, P,
                       (Signal*)signal_ptrs[rank], rank, p, plan, (const u32x4*)src, (u32x4*)out, epoch, epoch_dev);
  else
    hipLaunchKernelGGL(k_ipc_copy_plan<kPlanMaxPulls>, dim3(blocks), dim3(kIpcThreads), 0, (hipStream_t)stream, P,
                       (Signal*)signal_ptrs[rank], rank, p, plan, (const u32x4*)src, (u32x4*)out, epoch, epoch_dev);
  return (int)hipGetLastError();
}

extern "C" int mp4x_ipc_occupancy_misc(int family, int dtype, int p, int* blocks_per_cu) {
  int m = 1 << 30;
  int e = 0;
  if (family == 1) {
    occ_min(k_ipc_copy_plan<kIpcMaxRanks>, &m);       // the shared-GPU cap must hold for both forms
    occ_min(k_ipc_copy_plan<kPlanMaxPulls>, &m);
  } else {
    e = with_nr(p, [&](auto nrc) {
      constexpr int NR = decltype(nrc)::value;
      if (family == 0) {
        occ_min(k_ipc_gather<NR>, &m);
        return 0;
      }
      if (family == 4 || family == 5) {                  // the fp8 halves as collectives
        switch (dtype) {
          case MP4X_F32: family == 4 ? occ_min(k_ipc_fp8_rs<MP4X_F32, NR>, &m)
                                     : occ_min(k_ipc_fp8_ag<MP4X_F32, NR>, &m); return 0;
          case MP4X_BF16: family == 4 ? occ_min(k_ipc_fp8_rs<MP4X_BF16, NR>, &m)
                                      : occ_min(k_ipc_fp8_ag<MP4X_BF16, NR>, &m); return 0;
          case MP4X_F16: family == 4 ? occ_min(k_ipc_fp8_rs<MP4X_F16, NR>, &m)
                                     : occ_min(k_ipc_fp8_ag<MP4X_F16, NR>, &m); return 0;
          default: return (int)MP4X_E_UNSUPPORTED;
        }
      }
      if (family == 6) {                                 // the fp8 ragged all-to-all
        switch (dtype) {
          case MP4X_F32: occ_min(k_ipc_fp8_a2a<MP4X_F32, NR>, &m); return 0;
          case MP4X_BF16: occ_min(k_ipc_fp8_a2a<MP4X_BF16, NR>, &m); return 0;
          case MP4X_F16: occ_min(k_ipc_fp8_a2a<MP4X_F16, NR>, &m); return 0;
          default: return (int)MP4X_E_UNSUPPORTED;
        }
      }
      const bool narrow = family == 3;
      switch (dtype) {
        case MP4X_F32: narrow ? occ_min(k_ipc_fp8_twoshot_narrow<MP4X_F32, NR>, &m)
                              : occ_min(k_ipc_fp8_twoshot<MP4X_F32, NR>, &m); return 0;
        case MP4X_BF16: narrow ? occ_min(k_ipc_fp8_twoshot_narrow<MP4X_BF16, NR>, &m)
                               : occ_min(k_ipc_fp8_twoshot<MP4X_BF16, NR>, &m); return 0;
        case MP4X_F16: narrow ? occ_min(k_ipc_fp8_twoshot_narrow<MP4X_F16, NR>, &m)
                              : occ_min(k_ipc_fp8_twoshot<MP4X_F16, NR>, &m); return 0;
        default: return (int)MP4X_E_UNSUPPORTED;
      }
    });
  }
  *blocks_per_cu = m == (1 << 30) ? 0 : m;
  return e;
}
