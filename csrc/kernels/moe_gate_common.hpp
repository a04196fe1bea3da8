// What the two router-gate files share (moe_gate.hip: K10; moe_gate_group.hip: K13): the limits, the
// order-preserving key, the 64-bit shuffle, the row load, the sigmoid, the id load, the lane-group
// shape, the dtype / NV dispatch, the argument check and what a forward entry does around its launch
// (gate_forward).  The two forward kernels are separate and each keeps its own text; the one
// backward of both gates (k_moe_gate_bwd behind gate_backward) and k_moe_gate_stats are defined in
// moe_gate.hip and declared here.
#pragma once
#include "common.hpp"

namespace mp4x {

constexpr int kGateMaxE = 2048;      // K9's kMoeMaxNb
constexpr int kGateMaxK = 16;
constexpr int kGateMaxBlocks = 1024; // 4 blocks per CU; the statistics keep a partial per block
constexpr int kGateSlices = 32;      // of the second stage
constexpr int kGateCols = kBlock / kGateSlices;

// Unsigned order == float order, with -0 folded onto +0 (they compare equal).
__device__ __forceinline__ uint32_t gate_key(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0) u = 0;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float gate_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

__device__ __forceinline__ uint64_t gate_shfl_xor(uint64_t v, int off) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
  return ((uint64_t)hi << 32) | lo;
}

// The row of token t as floats: x[v * W + j] = column (sub + v * G) * W + j, or `fill` past E.
template <int DT, int NV>
__device__ __forceinline__ void gate_load_row(const void* __restrict__ logits, int64_t t, int E, int G, int sub, bool vec,
                                              bool valid, float fill, float (&x)[NV * (16 / (int)sizeof(typename Elem<DT>::S))]) {
  using S = typename Elem<DT>::S;
  constexpr int W = 16 / sizeof(S);
  const S* row = reinterpret_cast<const S*>(logits) + t * E;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c0 = (sub + v * G) * W;
    float a[W];
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] = fill;
    if (valid && c0 < E) {
      if (vec) {                         // E % W == 0: the vector is whole
        unpack<DT>(*reinterpret_cast<const u32x4*>(row + c0), a);
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (c0 + j < E) a[j] = Elem<DT>::load(row[c0 + j]);
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) x[v * W + j] = a[j];
  }
}

__device__ __forceinline__ float gate_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// prob_sum[e] / counts[e] from the nblk per-block partials; nblk == 0 writes zeros (moe_gate.hip).
__global__ __launch_bounds__(kBlock) void k_moe_gate_stats(const float* __restrict__ psum_part,
                                                           const int32_t* __restrict__ cnt_part, int nblk, int E,
                                                           float* __restrict__ prob_sum, int64_t* __restrict__ counts);

__device__ __forceinline__ int64_t gate_id(const void* __restrict__ ids, int is_i64, int64_t i) {
  return is_i64 ? reinterpret_cast<const int64_t*>(ids)[i] : (int64_t)reinterpret_cast<const int32_t*>(ids)[i];
}

// The backward of both gates (moe_gate.hip): k_moe_gate_bwd for the softmax (`sigmoid` 0: `lse` is
// needed) or the sigmoid score, after the entry has checked dtype, T, E, K and scale.
int gate_backward(int dtype, const void* logits, const float* lse, const void* ids, int ids_are_i64, int64_t T, int E, int K,
                  int sigmoid, int renormalize, float scale, const float* g_weights, const float* g_lse,
                  const float* g_prob_sum, void* g_logits, void* stream);

}  // namespace mp4x

namespace {
using namespace mp4x;

size_t gate_align(size_t x) { return (x + 255) & ~(size_t)255; }

int gate_dtype_ok(int dtype) { return (dtype == MP4X_F32 || dtype == MP4X_BF16 || dtype == MP4X_F16) ? 0 : MP4X_E_UNSUPPORTED; }

// The row's shape on the wave: G lanes per token (a power of two), NV vectors per lane.
struct GateShape {
  int G, lgG, NV, vec;
  int64_t nblk;
};

GateShape gate_shape(int dtype, int64_t T, int E) {
  const int W = 16 / elem_size(dtype);
  const int nvec = (E + W - 1) / W;
  GateShape s;
  // about 16 values per lane (4 f32 vectors, 2 of 16-bit elements) before the group widens: a lane
  // scans its own values far cheaper than the group's __shfl_xor tree grows by a level
  const int per_lane = W == 4 ? 4 : 2;
  const int want = (nvec + per_lane - 1) / per_lane;
  s.G = 1;
  s.lgG = 0;
  while (s.G < want && s.G < 64) {
    s.G <<= 1;
    ++s.lgG;
  }
  s.NV = 1;
  while (s.NV * s.G < nvec) s.NV <<= 1;
  s.vec = E % W == 0;
  const int64_t per_block = (int64_t)(kBlock / 64) * (64 / s.G);       // tokens
  s.nblk = (T + per_block - 1) / per_block;
  if (s.nblk > kGateMaxBlocks) s.nblk = kGateMaxBlocks;
  if (s.nblk < 1) s.nblk = 1;
  return s;
}

// f(IntC<NV>{}) for NV in {1, 2, 4, 8} with NV * W <= 32 values per lane.
template <int DT, typename F> int with_gate_nv(int NV, F&& f) {
  constexpr int W = 16 / sizeof(typename Elem<DT>::S);
  switch (NV) {
    case 1: return f(IntC<1>{});
    case 2: return f(IntC<2>{});
    case 4: return f(IntC<4>{});
    case 8:
      if constexpr (8 * W <= 32) return f(IntC<8>{});
      return MP4X_E_BADARG;
    default: return MP4X_E_BADARG;
  }
}

template <typename F> int with_gate_dtype(int dtype, F&& f) {
  switch (dtype) {
    case MP4X_F32: return f(IntC<MP4X_F32>{});
    case MP4X_BF16: return f(IntC<MP4X_BF16>{});
    case MP4X_F16: return f(IntC<MP4X_F16>{});
    default: return MP4X_E_UNSUPPORTED;
  }
}

int gate_args_ok(int dtype, int64_t T, int E, int K) {
  if (int e = gate_dtype_ok(dtype)) return e;
  if (E < 1 || E > kGateMaxE || K < 1 || K > kGateMaxK || K > E || T < 0 || T > INT32_MAX / 2 / K) return MP4X_E_BADARG;
  return 0;
}

// What a forward entry does around its kernel, after its own argument checks: the statistics'
// pointers (both or neither), T == 0 (zeros for the statistics, nothing else), the pointers every
// forward has (`others_ok`: the entry's own, looked at with T > 0 only), the split of the scratch,
// launch(IntC<DT>, IntC<NV>, STATS as a bool constant, LDS bytes, psum_part, cnt_part) on the shape
// `s`, and k_moe_gate_stats over the per-block partials.
template <typename F>
int gate_forward(int dtype, const GateShape& s, const void* logits, int64_t T, int E, float* weights, void* ids,
                 int ids_are_i64, bool others_ok, float* prob_sum, int64_t* counts, void* scratch, size_t scratch_bytes,
                 hipStream_t st, F&& launch) {
  const bool stats = prob_sum || counts;
  if (stats && (!prob_sum || !counts || ((uintptr_t)prob_sum & 3) || ((uintptr_t)counts & 7))) return MP4X_E_BADARG;
  const int scols = (E + kGateCols - 1) / kGateCols;
  if (T == 0) {
    if (!stats) return 0;
    hipLaunchKernelGGL(k_moe_gate_stats, dim3(scols), dim3(kBlock), 0, st, (const float*)nullptr, (const int32_t*)nullptr, 0,
                       E, prob_sum, counts);
    return (int)hipGetLastError();
  }
  if (!logits || ((uintptr_t)logits & 15) || !weights || ((uintptr_t)weights & 3) || !ids ||
      ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) || !others_ok)
    return MP4X_E_BADARG;
  float* psum_part = nullptr;
  int32_t* cnt_part = nullptr;
  if (stats) {
    if (!scratch || ((uintptr_t)scratch & 255) || scratch_bytes < mp4x_moe_gate_scratch_bytes(dtype, T, E))
      return MP4X_E_BADARG;
    psum_part = (float*)scratch;
    cnt_part = (int32_t*)((char*)scratch + gate_align((size_t)s.nblk * E * sizeof(float)));
  }
  const int e = with_gate_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    return with_gate_nv<DT>(s.NV, [&](auto nvc) {
      constexpr int VPL = decltype(nvc)::value * (16 / (int)sizeof(typename Elem<DT>::S));
      const size_t lds = (size_t)kBlock * VPL * sizeof(float) + (size_t)E * sizeof(int32_t);
      if (stats) launch(dtc, nvc, std::true_type{}, lds, psum_part, cnt_part);
      else launch(dtc, nvc, std::false_type{}, (size_t)0, psum_part, cnt_part);
      return (int)hipGetLastError();
    });
  });
  if (e || !stats) return e;
  hipLaunchKernelGGL(k_moe_gate_stats, dim3(scols), dim3(kBlock), 0, st, (const float*)psum_part, (const int32_t*)cnt_part,
                     (int)s.nblk, E, prob_sum, counts);
  return (int)hipGetLastError();
}
}  // namespace
