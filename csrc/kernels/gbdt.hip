// K16 — GBDT on the GPU in exact fixed point: quantise, histogram, best split (gfx950).
//
//   quantize  k_gbdt_quantize   gh[r] = (q(g[r], sg), q(h[r], sh)), q(x, s) = clamp(rint(f64(x) * 2^s)) with
//                               NaN -> 0: the product is a change of exponent (exact), one rounding to
//                               nearest even.  Two rows a lane, one 16-byte store
//   hist      k_gbdt_tables     one block: the raw segment table into LDS, then one lane runs
//                               gbdt_map::build_tables over it: c (clamped slot bounds) and T (tile
//                               bases), int32, into the scratch.  No host read of the table
//             k_gbdt_zero       hist = 0 (a kernel, so a captured graph holds no memset node)
//             k_gbdt_hist       a block per (tile of kTile row slots of one node, group of fg
//                               features): a private [fg, B, 2] int64 histogram in LDS, filled with
//                               64-bit LDS integer atomics, then its non-zero counters go to `hist`
//                               with 64-bit global integer atomics.  Lanes spread over features first
//                               (gbdt_hist_map.hpp): lane l takes feature l % fg of row l / fg, so the
//                               fg lanes of a row read fg adjacent bytes (one request, whatever the
//                               alignment of bins + r * F: single-byte loads assume none) and share
//                               one broadcast read of gh[r].  kUnroll rows a lane are gathered
//                               (rows[] -> bins[r, f], gh[r]) before the first is used
//   split     k_gbdt_split_feat a wave per (node, feature): 4 bins a lane, a wave scan of the int64
//                               (G, H) pairs, the gain in float64 without contraction, a wave argmax
//                               on (gain, -t): one record per (node, feature) in the scratch
//             k_gbdt_split_node a wave per node: the argmax of the records on (gain, -f)
//
// Why 64-bit counters: a row adds up to 2^31 - 1, so a 32-bit counter could hold one row; splitting a
// value into 16-bit parts so that kTile of them fit 32 bits takes four atomics where ds_add_u64 takes
// two.  Integer adds commute: the histogram has the same bits for every block schedule, tile size and
// rank count.  No float atomics, no host synchronisation, no allocation: recordable in a graph.
#include "common.hpp"
#include "gbdt_hist_map.hpp"

namespace mp4x {

namespace gm = gbdt_map;
static_assert(gm::kWaves * gm::kWave == kBlock, "a block is kWaves waves");

constexpr int kGbdtUnroll = 4;        // rows a lane gathers before it uses the first

__global__ __launch_bounds__(kBlock) void k_gbdt_quantize(const float* __restrict__ g, const float* __restrict__ h,
                                                          int64_t n, int sg, int sh, int32_t* __restrict__ gh) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
  if (r + 1 < n) {
    const float2 gv = *reinterpret_cast<const float2*>(g + r), hv = *reinterpret_cast<const float2*>(h + r);
    int4 o;
    o.x = gm::q(gv.x, sg);
    o.y = gm::q(hv.x, sh);
    o.z = gm::q(gv.y, sg);
    o.w = gm::q(hv.y, sh);
    *reinterpret_cast<int4*>(gh + 2 * r) = o;
  } else if (r < n) {
    int2 o;
    o.x = gm::q(g[r], sg);
    o.y = gm::q(h[r], sh);
    *reinterpret_cast<int2*>(gh + 2 * r) = o;
  }
}

// c = tab[0 .. k], T = tab[k + 1 .. 2k + 1].
__global__ __launch_bounds__(kBlock) void k_gbdt_tables(const int64_t* __restrict__ seg, int k, int64_t m,
                                                        int32_t* __restrict__ tab) {
  __shared__ int64_t raw[gm::kMaxNodes + 1];
  for (int j = threadIdx.x; j <= k; j += kBlock) raw[j] = seg[j];
  __syncthreads();
  if (threadIdx.x == 0) gm::build_tables(raw, k, m, tab, tab + k + 1);
}

__global__ __launch_bounds__(kBlock) void k_gbdt_zero(int64_t* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) p[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_gbdt_hist(const uint8_t* __restrict__ bins, const int32_t* __restrict__ gh,
                                                      const int32_t* __restrict__ rows, const int32_t* __restrict__ tab,
                                                      int64_t n, int64_t F, int B, int k, int64_t ngroups,
                                                      unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lh[];   // [fg][B][2]
  const int tid = threadIdx.x;
  const gm::Shape s = gm::shape(F, B);
  const gm::Tile t = gm::tile_of(tab, tab + k + 1, k, (int64_t)blockIdx.x, ngroups, F, s);
  if (!t.owns) return;                                   // block-uniform: before the first barrier
  const int cells = s.fg * B * 2;
  for (int j = tid; j < cells; j += kBlock) lh[j] = 0;
  __syncthreads();
  const int f = gm::lane_feature(s, t, tid);
  if (f >= 0) {
    const int step = gm::rows_per_step(s);
    unsigned long long* mine = lh + (size_t)(f - t.f0) * B * 2;
    for (int64_t i0 = (int64_t)t.lo + gm::lane_row(s, tid); i0 < t.hi; i0 += (int64_t)step * kGbdtUnroll) {
      int32_t r[kGbdtUnroll];
      int b[kGbdtUnroll];
      int2 v[kGbdtUnroll];
#pragma unroll
      for (int u = 0; u < kGbdtUnroll; ++u) {
        const int64_t i = i0 + (int64_t)u * step;
        r[u] = i < t.hi ? rows[i] : -1;
      }
#pragma unroll
      for (int u = 0; u < kGbdtUnroll; ++u) {
        const bool ok = r[u] >= 0 && (int64_t)r[u] < n;
        b[u] = ok ? (int)bins[(int64_t)r[u] * F + f] : gm::kMaxBins;
        v[u] = ok ? *reinterpret_cast<const int2*>(gh + 2 * (int64_t)r[u]) : make_int2(0, 0);
      }
#pragma unroll
      for (int u = 0; u < kGbdtUnroll; ++u) {
        if (b[u] < B) {
          atomicAdd(&mine[2 * b[u]], (unsigned long long)(long long)v[u].x);
          atomicAdd(&mine[2 * b[u] + 1], (unsigned long long)(long long)v[u].y);
        }
      }
    }
  }
  __syncthreads();
  const int64_t fb2 = (int64_t)B * 2;
  unsigned long long* out = hist + ((int64_t)t.node * F + t.f0) * fb2;
  const int live = (t.f1 - t.f0) * B * 2;               // the features of the tail group that exist
  for (int j = tid; j < live; j += kBlock) {
    const unsigned long long x = lh[j];
    if (x) atomicAdd(&out[j], x);
  }
}

// ---------------------------------------------------------------- best split
struct GbdtRec {          // one (node, feature): 48 bytes
  double gain;            // -inf: no finite gain
  int64_t t;
  int64_t GL, HL, G, H;
};

__device__ __forceinline__ double gbdt_real(int64_t x, int s) { return __builtin_ldexp((double)x, -s); }

// gain(f, t) in the order of the definition, every operation rounded once.
__device__ __forceinline__ double gbdt_gain(int64_t GL, int64_t HL, int64_t G, int64_t H, int sg, int sh, double lam) {
#pragma clang fp contract(off)
  const double gl = gbdt_real(GL, sg), hl = gbdt_real(HL, sh), gr = gbdt_real(G - GL, sg), hr = gbdt_real(H - HL, sh);
  const double gt = gbdt_real(G, sg), ht = gbdt_real(H, sh);
  const double a = gl * gl;
  const double b = hl + lam;
  const double left = a / b;
  const double c = gr * gr;
  const double d = hr + lam;
  const double right = c / d;
  const double both = left + right;
  const double e = gt * gt;
  const double q = ht + lam;
  const double whole = e / q;
  return both - whole;
}

__device__ __forceinline__ bool gbdt_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// (gain a, index ia) beats (gain b, index ib): the larger gain, then the lower index.
__device__ __forceinline__ bool gbdt_beats(double a, int64_t ia, double b, int64_t ib) {
  return a > b || (a == b && ia < ib);
}

constexpr int kGbdtBinsPerLane = gm::kMaxBins / 64;

__global__ __launch_bounds__(kBlock) void k_gbdt_split_feat(const int64_t* __restrict__ hist, int64_t nf, int B, int sg,
                                                            int sh, double lam, GbdtRec* __restrict__ rec) {
  const int64_t w = wave_id();
  if (w >= nf) return;                                  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t* hp = hist + w * B * 2;
  int64_t g[kGbdtBinsPerLane], h[kGbdtBinsPerLane];
  int64_t sumg = 0, sumh = 0;
#pragma unroll
  for (int j = 0; j < kGbdtBinsPerLane; ++j) {
    const int b = lane * kGbdtBinsPerLane + j;
    g[j] = b < B ? hp[2 * b] : 0;
    h[j] = b < B ? hp[2 * b + 1] : 0;
    sumg = (int64_t)((uint64_t)sumg + (uint64_t)g[j]);
    sumh = (int64_t)((uint64_t)sumh + (uint64_t)h[j]);
    g[j] = sumg;
    h[j] = sumh;
  }
  // inclusive wave scan of the lane totals
  int64_t ig = sumg, ih = sumh;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t og = __shfl_up((long long)ig, d), oh = __shfl_up((long long)ih, d);
    if (lane >= d) {
      ig = (int64_t)((uint64_t)ig + (uint64_t)og);
      ih = (int64_t)((uint64_t)ih + (uint64_t)oh);
    }
  }
  const int64_t G = __shfl((long long)ig, 63), H = __shfl((long long)ih, 63);
  const int64_t eg = (int64_t)((uint64_t)ig - (uint64_t)sumg), eh = (int64_t)((uint64_t)ih - (uint64_t)sumh);
  double best = -__builtin_inf();
  int64_t bt = gm::kMaxBins, bGL = 0, bHL = 0;
#pragma unroll
  for (int j = 0; j < kGbdtBinsPerLane; ++j) {
    const int b = lane * kGbdtBinsPerLane + j;
    const int64_t GL = (int64_t)((uint64_t)eg + (uint64_t)g[j]), HL = (int64_t)((uint64_t)eh + (uint64_t)h[j]);
    if (b <= B - 2) {
      const double x = gbdt_gain(GL, HL, G, H, sg, sh, lam);
      if (gbdt_finite(x) && gbdt_beats(x, b, best, bt)) {
        best = x;
        bt = b;
        bGL = GL;
        bHL = HL;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ox = __shfl_xor(best, d);
    const int64_t ot = __shfl_xor((long long)bt, d), oG = __shfl_xor((long long)bGL, d), oH = __shfl_xor((long long)bHL, d);
    if (gbdt_beats(ox, ot, best, bt)) {
      best = ox;
      bt = ot;
      bGL = oG;
      bHL = oH;
    }
  }
  if (lane == 0) {
    GbdtRec o;
    o.gain = best;
    o.t = bt;
    o.GL = bGL;
    o.HL = bHL;
    o.G = G;
    o.H = H;
    rec[w] = o;
  }
}

__global__ __launch_bounds__(kBlock) void k_gbdt_split_node(const GbdtRec* __restrict__ rec, int64_t k, int64_t F,
                                                            double* __restrict__ gain, int32_t* __restrict__ feature,
                                                            int32_t* __restrict__ threshold, int64_t* __restrict__ GL,
                                                            int64_t* __restrict__ HL, int64_t* __restrict__ G,
                                                            int64_t* __restrict__ H) {
  const int64_t w = wave_id();
  if (w >= k) return;
  const int lane = threadIdx.x & 63;
  const GbdtRec* rp = rec + w * F;
  double best = -__builtin_inf();
  int64_t bf = F;
  for (int64_t f = lane; f < F; f += 64) {
    const double x = rp[f].gain;
    if (gbdt_finite(x) && gbdt_beats(x, f, best, bf)) {
      best = x;
      bf = f;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ox = __shfl_xor(best, d);
    const int64_t of = __shfl_xor((long long)bf, d);
    if (gbdt_beats(ox, of, best, bf)) {
      best = ox;
      bf = of;
    }
  }
  if (lane == 0) {
    const bool split = bf < F && best > 1e-12;
    const GbdtRec r = rp[split ? bf : 0];
    gain[w] = best;
    feature[w] = split ? (int32_t)bf : -1;
    threshold[w] = split ? (int32_t)r.t : -1;
    GL[w] = split ? r.GL : 0;
    HL[w] = split ? r.HL : 0;
    G[w] = r.G;
    H[w] = r.H;
  }
}

}  // namespace mp4x

using namespace mp4x;

extern "C" int mp4x_gbdt_quantize(const float* g, const float* h, int64_t n, int shift_g, int shift_h, int32_t* gh,
                                  void* stream) {
  if (n < 0 || n >= gm::kMaxRows || shift_g < -gm::kMaxShift || shift_g > gm::kMaxShift || shift_h < -gm::kMaxShift ||
      shift_h > gm::kMaxShift)
    return MP4X_E_BADARG;
  if (n == 0) return 0;
  if (!g || ((uintptr_t)g & 7) || !h || ((uintptr_t)h & 7) || !gh || ((uintptr_t)gh & 15)) return MP4X_E_BADARG;
  const int64_t blocks = (n + 2 * kBlock - 1) / (2 * kBlock);
  hipLaunchKernelGGL(k_gbdt_quantize, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, g, h, n, shift_g,
                     shift_h, gh);
  return (int)hipGetLastError();
}

// c int32[k + 1] | T int32[k + 1].
extern "C" size_t mp4x_gbdt_hist_scratch_bytes(int k) {
  if (k < 0 || k > gm::kMaxNodes) return 0;
  return (size_t)(2 * (k + 1)) * sizeof(int32_t);
}

extern "C" int mp4x_gbdt_hist(const uint8_t* bins, const int32_t* gh, const int32_t* rows, const int64_t* seg, int64_t n,
                              int64_t F, int B, int64_t m, int k, int64_t* hist, void* scratch, size_t scratch_bytes,
                              void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= gm::kMaxRows || m < 0 || m >= gm::kMaxRows || F < 1 || F > INT32_MAX || B < 2 || B > gm::kMaxBins ||
      k < 0 || k > gm::kMaxNodes)
    return MP4X_E_BADARG;
  if (k == 0) return 0;
  if (!hist || ((uintptr_t)hist & 7) || !seg || ((uintptr_t)seg & 7)) return MP4X_E_BADARG;
  const int64_t cells = (int64_t)k * F * B * 2;
  if (cells >= gm::kMaxRows * 2) return MP4X_E_BADARG;
  hipLaunchKernelGGL(k_gbdt_zero, dim3(grid_for(cells, 4)), dim3(kBlock), 0, st, hist, cells);
  if (int e = (int)hipGetLastError()) return e;
  if (m == 0 || n == 0) return 0;
  if (!bins || !gh || ((uintptr_t)gh & 7) || !rows || ((uintptr_t)rows & 3) || !scratch || ((uintptr_t)scratch & 3) ||
      scratch_bytes < mp4x_gbdt_hist_scratch_bytes(k))
    return MP4X_E_BADARG;
  const gm::Shape s = gm::shape(F, B);
  const int64_t ngroups = gm::groups(F, s.fg), grid = gm::max_tiles(m, k) * ngroups;
  if (grid > INT32_MAX) return MP4X_E_BADARG;
  int32_t* tab = (int32_t*)scratch;
  hipLaunchKernelGGL(k_gbdt_tables, dim3(1), dim3(kBlock), 0, st, seg, k, m, tab);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_gbdt_hist, dim3((unsigned)grid), dim3(kBlock), (size_t)s.fg * B * 16, st, bins, gh, rows,
                     (const int32_t*)tab, n, F, B, k, ngroups, (unsigned long long*)hist);
  return (int)hipGetLastError();
}

extern "C" size_t mp4x_gbdt_split_scratch_bytes(int64_t k, int64_t F) {
  if (k < 0 || F < 1 || k * F >= gm::kMaxRows) return 0;
  return (size_t)(k * F) * sizeof(GbdtRec);
}

extern "C" int mp4x_gbdt_split(const int64_t* hist, int64_t k, int64_t F, int B, int shift_g, int shift_h, double lam,
                               double* gain, int32_t* feature, int32_t* threshold, int64_t* GL, int64_t* HL, int64_t* G,
                               int64_t* H, void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (k < 0 || F < 1 || B < 2 || B > gm::kMaxBins || k * F >= gm::kMaxRows || shift_g < -gm::kMaxShift ||
      shift_g > gm::kMaxShift || shift_h < -gm::kMaxShift || shift_h > gm::kMaxShift)
    return MP4X_E_BADARG;
  if (k == 0) return 0;
  if (!hist || ((uintptr_t)hist & 7) || !gain || ((uintptr_t)gain & 7) || !feature || ((uintptr_t)feature & 3) ||
      !threshold || ((uintptr_t)threshold & 3) || !GL || ((uintptr_t)GL & 7) || !HL || ((uintptr_t)HL & 7) || !G ||
      ((uintptr_t)G & 7) || !H || ((uintptr_t)H & 7) || !scratch || ((uintptr_t)scratch & 7) ||
      scratch_bytes < mp4x_gbdt_split_scratch_bytes(k, F))
    return MP4X_E_BADARG;
  GbdtRec* rec = (GbdtRec*)scratch;
  const int64_t nf = k * F, wpb = kBlock / 64;
  hipLaunchKernelGGL(k_gbdt_split_feat, dim3((unsigned)((nf + wpb - 1) / wpb)), dim3(kBlock), 0, st, hist, nf, B, shift_g,
                     shift_h, lam, rec);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(k_gbdt_split_node, dim3((unsigned)((k + wpb - 1) / wpb)), dim3(kBlock), 0, st, (const GbdtRec*)rec, k,
                     F, gain, feature, threshold, GL, HL, G, H);
  return (int)hipGetLastError();
}
