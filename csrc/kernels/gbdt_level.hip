// K17 — GBDT level advance on the GPU: stable two-way row partition and sibling subtraction (gfx950,
// integers only).
//
// The rows of a level arrive grouped by parent node (rows int32[m] under a K16 segment table).  The
// next grouping is a stable two-way partition inside every segment: count / offsets / scatter, the
// halves of K4b/K9 with two buckets, over gbdt_hist_map.hpp's tiles (one feature group) and
// gbdt_part_map.hpp's destinations.
//
//   k_gbdt_tables2       one block: the raw table into LDS, one lane runs gbdt_map::build_tables
//   k_gbdt_part_count    a block per tile, a wave per 16 consecutive wave steps: each lane loads
//                        rows[i], tests the range and gathers the one byte bins[r, f] of the node's
//                        split feature; kUnroll steps' row ids and bytes are loaded before the first
//                        is used.  Two ballots a step are the first / second masks: kept in lane
//                        `step` and stored as one 256-byte run a wave (2 bits a slot), so the byte
//                        gather - one byte used of a whole request - happens once.  The block's two
//                        counts go to the scan arrays
//   k_gbdt_part_offsets  one block: exclusive scans of the per-tile first and second counts in tile
//                        order, kScan tiles a pass, in place; node boundaries are read out of the
//                        scans (tile order is node-major): seg2
//   k_gbdt_part_scatter  a block per tile: lane l of every wave loads the mask pair of step l (1 KiB a
//                        tile), a wave scan of the popcounts gives every step's prefix, so no LDS and
//                        no barrier; a slot goes to base + prefix + popcount(mask & lower lanes).
//                        Reads rows and masks only
//   k_gbdt_hist_sub      large[p] = parent[parent_of[p]] - small[p]: a (g, h) int64 pair a lane step,
//                        16-byte loads and stores, grid-stride inside a node (blockIdx.y = p)
//
// No block waits on another, no global atomic, no host read of the table, no allocation: every
// launch is on the caller's stream and recordable in a graph.  Order comes from the prefix, so the
// output has the same bits run to run.
#include "common.hpp"
#include "gbdt_part_map.hpp"

namespace mp4x {

namespace gm = gbdt_map;
namespace gp = gbdt_part;
static_assert(gm::kWaves * gm::kWave == kBlock && gp::kScan == kBlock, "a block is kWaves waves, one scan pass");

constexpr int kPartUnroll = 4;        // steps whose row ids and bytes a lane loads before it uses the first
static_assert(gp::kWaveSteps % kPartUnroll == 0, "whole unrolled trips");

// c = tab[0 .. k], T = tab[k + 1 .. 2k + 1] (gbdt.hip's k_gbdt_tables, at most kMaxParents nodes).
__global__ __launch_bounds__(kBlock) void k_gbdt_tables2(const int64_t* __restrict__ seg, int k, int64_t m,
                                                         int32_t* __restrict__ tab) {
  __shared__ int64_t raw[gp::kMaxParents + 1];
  for (int j = threadIdx.x; j <= k; j += kBlock) raw[j] = seg[j];
  __syncthreads();
  if (threadIdx.x == 0) gm::build_tables(raw, k, m, tab, tab + k + 1);
}

__global__ __launch_bounds__(kBlock) void k_gbdt_zero_seg(int64_t* __restrict__ seg_out, int n) {
  for (int j = threadIdx.x; j < n; j += kBlock) seg_out[j] = 0;
}

__global__ __launch_bounds__(kBlock) void k_gbdt_part_count(
    const uint8_t* __restrict__ bins, const int32_t* __restrict__ rows, const int32_t* __restrict__ tab,
    const int32_t* __restrict__ feature, const int32_t* __restrict__ threshold, const int32_t* __restrict__ first_right,
    int64_t n, int64_t F, int k, int64_t tiles, ulonglong2* __restrict__ masks, int32_t* __restrict__ scan) {
  __shared__ int wc[2][gm::kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const gm::Shape one = {1, 0, gm::kWave};
  const gm::Tile t = gm::tile_of(tab, tab + k + 1, k, (int64_t)blockIdx.x, 1, F, one);
  gp::Rule r = gp::rule(-1, 0, 0, F);
  if (t.owns) r = gp::rule(feature[t.node], threshold[t.node], first_right ? first_right[t.node] : 0, F);
  unsigned long long keep_f = 0, keep_s = 0;
  int nf = 0, ns = 0;
  if (t.owns && r.splits) {                              // block-uniform: whole waves ballot
    const int s_lo = gp::first_step(wave);
    for (int s0 = 0; s0 < gp::kWaveSteps; s0 += kPartUnroll) {
      if (gp::slot_of(t, s_lo + s0, 0) >= t.hi) break;   // wave-uniform: the rest of the wave's run is past the end
      int32_t row[kPartUnroll];
      int bin[kPartUnroll];
#pragma unroll
      for (int u = 0; u < kPartUnroll; ++u) {
        const int64_t i = gp::slot_of(t, s_lo + s0 + u, lane);
        row[u] = i < t.hi ? rows[i] : -1;
      }
#pragma unroll
      for (int u = 0; u < kPartUnroll; ++u) {
        const bool ok = row[u] >= 0 && (int64_t)row[u] < n;
        bin[u] = ok ? (int)bins[(int64_t)row[u] * F + r.f] : -1;
      }
#pragma unroll
      for (int u = 0; u < kPartUnroll; ++u) {
        const int sd = gp::side(r, bin[u]);
        const unsigned long long fm = __ballot(sd == 1), sm = __ballot(sd == 2);
        nf += gp::bits(fm);
        ns += gp::bits(sm);
        if (lane == s0 + u) {
          keep_f = fm;
          keep_s = sm;
        }
      }
    }
  }
  if (t.owns && lane < gp::kWaveSteps)
    masks[(int64_t)blockIdx.x * gp::kSteps + gp::first_step(wave) + lane] = make_ulonglong2(keep_f, keep_s);
  if (lane == 0) {
    wc[0][wave] = nf;
    wc[1][wave] = ns;
  }
  __syncthreads();
  if (tid < 2) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < gm::kWaves; ++w) sum += wc[tid][w];
    scan[(int64_t)tid * (tiles + 1) + blockIdx.x] = sum;   // a tile that owns nothing counts 0
  }
}

// S = scan[0 .. tiles], G = scan[tiles + 1 .. 2 tiles + 1]: counts in, exclusive scans and totals out.
__global__ __launch_bounds__(kBlock) void k_gbdt_part_offsets(const int32_t* __restrict__ tab, int k, int64_t tiles,
                                                              int32_t* scan, int64_t* __restrict__ seg_out) {
  __shared__ int32_t ws[2][gm::kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* S = scan;
  int32_t* G = scan + tiles + 1;
  int32_t run_s = 0, run_g = 0;                          // the same in every thread
  const int64_t passes = gp::scan_passes(tiles);
  for (int64_t p = 0; p < passes; ++p) {
    const int64_t t = p * gp::kScan + tid;
    const int32_t a = t < tiles ? S[t] : 0, b = t < tiles ? G[t] : 0;
    int32_t ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t oa = __shfl_up(ia, d), ob = __shfl_up(ib, d);
      if (lane >= d) {
        ia += oa;
        ib += ob;
      }
    }
    if (lane == 63) {
      ws[0][wave] = ia;
      ws[1][wave] = ib;
    }
    __syncthreads();
    int32_t pa = 0, pb = 0, ta = 0, tb = 0;
#pragma unroll
    for (int w = 0; w < gm::kWaves; ++w) {
      if (w < wave) {
        pa += ws[0][w];
        pb += ws[1][w];
      }
      ta += ws[0][w];
      tb += ws[1][w];
    }
    if (t < tiles) {
      S[t] = run_s + pa + ia - a;
      G[t] = run_g + pb + ib - b;
    }
    run_s += ta;
    run_g += tb;
    __syncthreads();                                     // ws is read before the next pass writes it
  }
  if (tid == 0) {
    S[tiles] = run_s;
    G[tiles] = run_g;
  }
  __syncthreads();
  const int32_t* T = tab + k + 1;
  for (int j = tid; j <= k; j += kBlock) {
    const int64_t tj = gp::scan_index(T[j], tiles);
    if (j < k) seg_out[j] = S[tj];
    seg_out[k + j] = (int64_t)run_s + G[tj];             // j = 0: Stot = S[T[k]], every later tile is empty
  }
}

__global__ __launch_bounds__(kBlock) void k_gbdt_part_scatter(const int32_t* __restrict__ rows,
                                                              const int32_t* __restrict__ tab, int64_t F, int64_t m, int k,
                                                              int64_t tiles, const ulonglong2* __restrict__ masks,
                                                              const int32_t* __restrict__ scan,
                                                              int32_t* __restrict__ rows_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const gm::Shape one = {1, 0, gm::kWave};
  const gm::Tile t = gm::tile_of(tab, tab + k + 1, k, (int64_t)blockIdx.x, 1, F, one);
  if (!t.owns) return;
  const ulonglong2 mk = masks[(int64_t)blockIdx.x * gp::kSteps + lane];      // lane l: step l of the tile
  const int cf = gp::bits(mk.x), cs = gp::bits(mk.y);
  int ef = cf, es = cs;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int of = __shfl_up(ef, d), os = __shfl_up(es, d);
    if (lane >= d) {
      ef += of;
      es += os;
    }
  }
  ef -= cf;                                              // the bits of the steps before step `lane`
  es -= cs;
  const int64_t base_f = scan[blockIdx.x], base_s = (int64_t)scan[tiles] + scan[tiles + 1 + blockIdx.x];
  const int s_lo = gp::first_step(wave);
  for (int s0 = 0; s0 < gp::kWaveSteps; s0 += kPartUnroll) {
    if (gp::slot_of(t, s_lo + s0, 0) >= t.hi) break;     // wave-uniform
    int32_t row[kPartUnroll];
#pragma unroll
    for (int u = 0; u < kPartUnroll; ++u) {
      const int64_t i = gp::slot_of(t, s_lo + s0 + u, lane);
      row[u] = i < t.hi ? rows[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < kPartUnroll; ++u) {
      const int s = s_lo + s0 + u;
      const unsigned long long fm = __shfl(mk.x, s), sm = __shfl(mk.y, s);
      const int pf = __shfl(ef, s), ps = __shfl(es, s);
      const bool first = (fm >> lane) & 1, second = (sm >> lane) & 1;
      const int64_t d = first ? gp::dest(base_f, pf, fm, lane) : gp::dest(base_s, ps, sm, lane);
      if ((first || second) && gp::writable(d, m)) rows_out[d] = row[u];
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_gbdt_hist_sub(const longlong2* __restrict__ parent,
                                                          const longlong2* small,
                                                          const int32_t* __restrict__ parent_of, int k, int64_t cells,
                                                          longlong2* large) {
  const int64_t p = blockIdx.y;
  const int32_t j = parent_of[p];
  const bool has = j >= 0 && j < k;                      // block-uniform; outside: a zero histogram
  const longlong2* pp = parent + (has ? (int64_t)j * cells : 0);
  const longlong2* sp = small + p * cells;
  longlong2* lp = large + p * cells;
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (int64_t)gridDim.x * kBlock) {
    const longlong2 a = has ? pp[c] : make_longlong2(0, 0), b = sp[c];
    longlong2 o;
    o.x = (long long)((unsigned long long)a.x - (unsigned long long)b.x);
    o.y = (long long)((unsigned long long)a.y - (unsigned long long)b.y);
    lp[c] = o;
  }
}

static bool overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return an && bn && x < y + bn && y < x + an;
}

}  // namespace mp4x

using namespace mp4x;

extern "C" size_t mp4x_gbdt_partition_scratch_bytes(int64_t m, int k) {
  if (m < 0 || m >= gm::kMaxRows || k < 0 || k > gp::kMaxParents) return 0;
  return (size_t)gp::layout(m, k).bytes;
}

extern "C" int mp4x_gbdt_partition(const uint8_t* bins, const int32_t* rows, const int64_t* seg, const int32_t* feature,
                                   const int32_t* threshold, const int32_t* first_right, int64_t n, int64_t F, int64_t m,
                                   int k, int32_t* rows_out, int64_t* seg_out, void* scratch, size_t scratch_bytes,
                                   void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= gm::kMaxRows || m < 0 || m >= gm::kMaxRows || F < 1 || F > INT32_MAX || k < 0 || k > gp::kMaxParents)
    return MP4X_E_BADARG;
  if (!seg_out || ((uintptr_t)seg_out & 7)) return MP4X_E_BADARG;
  if (k == 0 || m == 0 || n == 0) {                      // no row can move: the table alone, all zero
    hipLaunchKernelGGL(k_gbdt_zero_seg, dim3(1), dim3(kBlock), 0, st, seg_out, 2 * k + 1);
    return (int)hipGetLastError();
  }
  const gp::Layout l = gp::layout(m, k);
  if (!bins || !rows || ((uintptr_t)rows & 3) || !seg || ((uintptr_t)seg & 7) || !feature || ((uintptr_t)feature & 3) ||
      !threshold || ((uintptr_t)threshold & 3) || ((uintptr_t)first_right & 3) || !rows_out || ((uintptr_t)rows_out & 3) ||
      !scratch || ((uintptr_t)scratch & 15) || scratch_bytes < l.bytes || l.tiles > INT32_MAX ||
      overlap(rows, (uint64_t)m * 4, rows_out, (uint64_t)m * 4))
    return MP4X_E_BADARG;
  ulonglong2* masks = (ulonglong2*)scratch;
  int32_t* tab = (int32_t*)((char*)scratch + l.tab);
  int32_t* scan = (int32_t*)((char*)scratch + l.scan);
  hipLaunchKernelGGL(k_gbdt_tables2, dim3(1), dim3(kBlock), 0, st, seg, k, m, tab);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_gbdt_part_count, dim3((unsigned)l.tiles), dim3(kBlock), 0, st, bins, rows, (const int32_t*)tab,
                     feature, threshold, first_right, n, F, k, l.tiles, masks, scan);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_gbdt_part_offsets, dim3(1), dim3(kBlock), 0, st, (const int32_t*)tab, k, l.tiles, scan, seg_out);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_gbdt_part_scatter, dim3((unsigned)l.tiles), dim3(kBlock), 0, st, rows, (const int32_t*)tab, F, m, k,
                     l.tiles, (const ulonglong2*)masks, (const int32_t*)scan, rows_out);
  return (int)hipGetLastError();
}

extern "C" int mp4x_gbdt_hist_subtract(const int64_t* parent, const int64_t* small, const int32_t* parent_of, int k, int kp,
                                       int64_t cells, int64_t* large, void* stream) {
  if (k < 0 || k > gm::kMaxNodes || kp < 0 || kp > gm::kMaxNodes || cells < 1 || cells >= gm::kMaxRows) return MP4X_E_BADARG;
  if (kp == 0) return 0;
  if ((k && !parent) || ((uintptr_t)parent & 15) || !small || ((uintptr_t)small & 15) || !parent_of ||
      ((uintptr_t)parent_of & 3) || !large || ((uintptr_t)large & 15) ||
      overlap(large, (uint64_t)kp * cells * 16, parent, (uint64_t)k * cells * 16))
    return MP4X_E_BADARG;
  hipLaunchKernelGGL(k_gbdt_hist_sub, dim3((unsigned)grid_for(cells), (unsigned)kp), dim3(kBlock), 0, (hipStream_t)stream,
                     (const longlong2*)parent, (const longlong2*)small, parent_of, k, cells, (longlong2*)large);
  return (int)hipGetLastError();
}
