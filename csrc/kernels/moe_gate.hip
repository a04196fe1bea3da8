// K10 — the fused top-k router gate of a mixture-of-experts layer (gfx950): softmax, top-k, the
// optional renormalisation over the chosen K and the router statistics in one pass over the
// logits [T, E]; the backward pass in one more.
//
// A token's row is spread over a lane group of G lanes (G = 1 .. 64, a power of two chosen from the
// row's 16-byte vectors as K9's lane_group does, at about 16 values per lane): 64 / G tokens per wave.  Lane `sub` of a group
// owns the vectors sub, sub + G, ... of the row (NV of them, a template argument: the VPL = NV * W
// values a lane holds stay in registers), i.e. the columns (sub + v * G) * W + j.  A row whose
// byte length is a whole number of vectors is loaded as 16-byte vectors, any other row as scalars
// of the same columns.
//
//   forward   k_moe_gate_fwd   every logit becomes a 32-bit key whose unsigned order is the float
//             order (-0 == +0; a NaN sorts above +inf or below -inf by its sign: any bits have a
//             place).  K rounds of a group-wide argmax (__shfl_xor tree) over (key, column) pairs,
//             greater key or equal key and smaller column; the owner lane retires the winner.  The
//             first winner is the row maximum m; sum = sum_j exp(l_j - m) (lane partials in column
//             order, then the tree), lse = m + log(sum), p = exp(l - m) / sum.
//             Statistics: a lane adds p of its columns over the wave's tokens (registers), the
//             64 / G groups of a wave and the 4 waves of a block are joined through LDS in (wave,
//             group) order, per-block partials go to scratch; the chosen ids are counted in an LDS
//             histogram (integer atomics) and go to scratch the same way.
//   stats     k_moe_gate_stats  prob_sum[e] and counts[e] from the per-block partials: 32 slices
//             of consecutive blocks, each summed in block order, joined in slice order.
//   backward  k_moe_gate_bwd   p_j = exp(l_j - lse) again from the saved logits and lse, the K
//             chosen probabilities from K more (cached) loads, then the closed form of
//             softmax + top-k + renormalisation + lse + prob_sum, rounded once to the logits' dtype.
//             The same kernel is K13's backward (moe_gate_group.hip): a scale on the gate weights'
//             gradient (1 here: exact) and, as a template argument, the sigmoid score, with
//             d_j = sigmoid(l_j) * sigmoid(-l_j), no lse and no dot over the row.
//
// No floating-point atomics and no global atomics at all: every result is identical run to run.
#include "moe_gate_common.hpp"

namespace mp4x {

template <int DT, int NV, bool STATS>
__global__ __launch_bounds__(kBlock) void k_moe_gate_fwd(const void* __restrict__ logits, int64_t T, int E, int K, int G,
                                                         int lgG, int vec, int renorm, float* __restrict__ weights,
                                                         void* __restrict__ ids, int ids_are_i64,
                                                         float* __restrict__ lse, float* __restrict__ psum_part,
                                                         int32_t* __restrict__ cnt_part) {
  using S = typename Elem<DT>::S;
  constexpr int W = 16 / sizeof(S);
  constexpr int LGW = W == 4 ? 2 : 3;
  constexpr int VPL = NV * W;
  static_assert(VPL <= 32, "the alive mask is 32 bits");
  extern __shared__ __attribute__((aligned(16))) char gate_smem[];
  float* lp = reinterpret_cast<float*>(gate_smem);                         // [4 * R][G * VPL] (STATS)
  int32_t* lh = reinterpret_cast<int32_t*>(gate_smem + (size_t)kBlock * VPL * sizeof(float));   // [E]
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = lane >> lgG, sub = lane & (G - 1), R = 64 >> lgG;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;

  float acc[VPL];
  if constexpr (STATS) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) acc[i] = 0.0f;
    for (int e = tid; e < E; e += kBlock) lh[e] = 0;
    __syncthreads();
  }

  // wave-uniform trip count: a group past T computes on a dead row and stores nothing
  for (int64_t t0 = wave * R; t0 < T; t0 += nwaves * R) {
    const int64_t t = t0 + grp;
    const bool valid = t < T;
    float x[VPL];
    gate_load_row<DT, NV>(logits, t, E, G, sub, vec != 0, valid, 0.0f, x);
    uint32_t key[VPL];
    uint32_t alive = 0;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      key[i] = gate_key(x[i]);
      if ((sub + (i / W) * G) * W + (i % W) < E) alive |= 1u << i;
    }

    float pk[kGateMaxK];
    int idk[kGateMaxK];
    float m = 0.0f, sum = 1.0f;
#pragma unroll
    for (int k = 0; k < kGateMaxK; ++k) {
      if (k >= K) continue;
      // (key, column) of the lane's best live value: a dead slot is 0, below every live pair
      uint64_t best = 0;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const uint32_t col = (uint32_t)((sub + (i / W) * G) * W + (i % W));
        const uint64_t c = ((alive >> i) & 1u) ? (((uint64_t)key[i] << 32) | (0xffffffffu - col)) : 0;
        best = c > best ? c : best;
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint64_t o = gate_shfl_xor(best, off);
        best = o > best ? o : best;
      }
      // K <= E live columns and one retired per round: a live pair always wins.  The clamp holds
      // the id inside [0, E) whatever happens.
      int col = (int)(0xffffffffu - (uint32_t)best);
      MP4X_DASSERT(col >= 0 && col < E);
      col = col < 0 ? 0 : (col >= E ? E - 1 : col);
      const float val = gate_unkey((uint32_t)(best >> 32));
      const int vi = col >> LGW;
      if (sub == (vi & (G - 1))) alive &= ~(1u << (((vi >> lgG) << LGW) | (col & (W - 1))));
      if (k == 0) {
        m = val;
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const bool in = (sub + (i / W) * G) * W + (i % W) < E;
          part += in ? expf(x[i] - m) : 0.0f;
        }
        for (int off = G >> 1; off >= 1; off >>= 1) part += __shfl_xor(part, off);
        sum = part;
      }
      pk[k] = expf(val - m) / sum;
      idk[k] = col;
    }

    float s = 1.0f;
    if (renorm) {
      s = 0.0f;
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        s += pk[k];
      }
    }
    if (valid) {
      if (sub == 0) lse[t] = m + logf(sum);
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        if ((k & (G - 1)) == sub) {
          const int64_t a = t * K + k;
          weights[a] = renorm ? pk[k] / s : pk[k];
          if (ids_are_i64) reinterpret_cast<int64_t*>(ids)[a] = idk[k];
          else reinterpret_cast<int32_t*>(ids)[a] = idk[k];
          if constexpr (STATS) atomicAdd(&lh[idk[k]], 1);
        }
      }
      if constexpr (STATS) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const bool in = (sub + (i / W) * G) * W + (i % W) < E;
          acc[i] += in ? expf(x[i] - m) / sum : 0.0f;
        }
      }
    }
  }

  if constexpr (STATS) {
    const int stride = G * VPL;                                   // >= E; 4 * R * stride = kBlock * VPL
    float* mine = lp + (size_t)((tid >> 6) * R + grp) * stride;
#pragma unroll
    for (int i = 0; i < VPL; ++i) mine[(sub + (i / W) * G) * W + (i % W)] = acc[i];
    __syncthreads();
    for (int e = tid; e < E; e += kBlock) {
      float a = 0.0f;
      for (int q = 0; q < 4 * R; ++q) a += lp[(size_t)q * stride + e];          // (wave, group) order
      psum_part[(int64_t)blockIdx.x * E + e] = a;
      cnt_part[(int64_t)blockIdx.x * E + e] = lh[e];
    }
  }
}

// prob_sum[e] / counts[e] from the nblk per-block partials; nblk == 0 writes zeros.
__global__ __launch_bounds__(kBlock) void k_moe_gate_stats(const float* __restrict__ psum_part,
                                                           const int32_t* __restrict__ cnt_part, int nblk, int E,
                                                           float* __restrict__ prob_sum, int64_t* __restrict__ counts) {
  __shared__ float sf[kGateSlices][kGateCols];
  __shared__ int64_t si[kGateSlices][kGateCols];
  const int c = threadIdx.x % kGateCols, sl = threadIdx.x / kGateCols;
  const int e = blockIdx.x * kGateCols + c;
  const int per = (nblk + kGateSlices - 1) / kGateSlices;
  const int b0 = sl * per, b1 = (b0 + per) < nblk ? (b0 + per) : nblk;
  float f = 0.0f;
  int64_t n = 0;
  if (e < E) {
    for (int b = b0; b < b1; ++b) {
      f += psum_part[(int64_t)b * E + e];
      n += cnt_part[(int64_t)b * E + e];
    }
  }
  sf[sl][c] = f;
  si[sl][c] = n;
  __syncthreads();
  if (sl == 0 && e < E) {
    f = 0.0f;
    n = 0;
    for (int q = 0; q < kGateSlices; ++q) {
      f += sf[q][c];
      n += si[q][c];
    }
    prob_sum[e] = f;
    counts[e] = n;
  }
}


// The backward of K10 (SIGMOID false) and of K13 (either score; the groups and the bias have no
// gradient): the gradient of the gate weights is scaled by `scale`, the sigmoid score has no lse
// and its columns do not depend on each other (no dot over the row).
template <int DT, int NV, bool SIGMOID>
__global__ __launch_bounds__(kBlock) void k_moe_gate_bwd(const void* __restrict__ logits, const float* __restrict__ lse,
                                                         const void* __restrict__ ids, int ids_are_i64, int64_t T,
                                                         int E, int K, int G, int lgG, int vec, int renorm, float scale,
                                                         const float* __restrict__ g_w, const float* __restrict__ g_lse,
                                                         const float* __restrict__ g_psum, void* __restrict__ g_logits) {
  using S = typename Elem<DT>::S;
  constexpr int W = 16 / sizeof(S);
  constexpr int VPL = NV * W;
  const int lane = threadIdx.x & 63;
  const int grp = lane >> lgG, sub = lane & (G - 1), R = 64 >> lgG;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;

  float gps[VPL];                                     // g_psum of the lane's columns: the same for every token
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int col = (sub + (i / W) * G) * W + (i % W);
    gps[i] = (g_psum && col < E) ? g_psum[col] : 0.0f;
  }

  for (int64_t t0 = wave * R; t0 < T; t0 += nwaves * R) {
    const int64_t t = t0 + grp;
    const bool valid = t < T;
    const int64_t tt = valid ? t : 0;                 // a group past T walks token 0 and stores nothing
    float x[VPL];
    gate_load_row<DT, NV>(logits, tt, E, G, sub, vec != 0, true, -INFINITY, x);      // -inf past E: score 0 there
    const float l = SIGMOID ? 0.0f : lse[tt];
    const float gl = (g_lse && !SIGMOID) ? g_lse[tt] : 0.0f;

    // the chosen K: their scores again (softmax: p_k = exp(l[id_k] - lse)); the lanes of a group
    // read the same (cached) words
    float pk[kGateMaxK], gq[kGateMaxK];
    int idk[kGateMaxK];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < kGateMaxK; ++k) {
      if (k >= K) continue;
      const int64_t id = gate_id(ids, ids_are_i64, tt * K + k);
      MP4X_DASSERT(id >= 0 && id < E);
      const bool ok = id >= 0 && id < E;              // an id outside the row takes no part and is never read through
      idk[k] = ok ? (int)id : -1;
      const float lk = ok ? Elem<DT>::load(reinterpret_cast<const S*>(logits)[tt * E + idk[k]]) : 0.0f;
      pk[k] = ok ? (SIGMOID ? gate_sigmoid(lk) : expf(lk - l)) : 0.0f;
      gq[k] = (g_w && ok) ? g_w[tt * K + k] : 0.0f;
      s += pk[k];
    }
    if (renorm) {
      float dw = 0.0f;
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        dw += gq[k] * (pk[k] / s);
      }
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        gq[k] = (gq[k] - dw) / s;
      }
    }
#pragma unroll
    for (int k = 0; k < kGateMaxK; ++k) {
      if (k >= K) continue;
      gq[k] *= scale;
    }

    float p[VPL], gp[VPL];
    float dot = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int col = (sub + (i / W) * G) * W + (i % W);
      // sigmoid: d = sigmoid(l) * sigmoid(-l), both by the forward's formula
      p[i] = SIGMOID ? gate_sigmoid(x[i]) * gate_sigmoid(-x[i]) : expf(x[i] - l);
      float g = gps[i];
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        g += idk[k] == col ? gq[k] : 0.0f;            // the ids of a token are distinct: one k at most
      }
      gp[i] = g;
      if constexpr (!SIGMOID) dot += col < E ? g * p[i] : 0.0f;
    }
    if constexpr (!SIGMOID) {
      for (int off = G >> 1; off >= 1; off >>= 1) dot += __shfl_xor(dot, off);
    }

    if (!valid) continue;
    S* out = reinterpret_cast<S*>(g_logits) + t * E;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int c0 = (sub + v * G) * W;
      if (c0 >= E) continue;
      float a[W];
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const int i = v * W + j;
        a[j] = SIGMOID ? p[i] * gp[i] : p[i] * (gp[i] - dot) + gl * p[i];
      }
      if (vec) {
        *reinterpret_cast<u32x4*>(out + c0) = pack<DT, u32x4>(a);
      } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
          if (c0 + j < E) out[c0 + j] = Elem<DT>::store(a[j]);
      }
    }
  }
}

int gate_backward(int dtype, const void* logits, const float* lse, const void* ids, int ids_are_i64, int64_t T, int E, int K,
                  int sigmoid, int renormalize, float scale, const float* g_weights, const float* g_lse,
                  const float* g_prob_sum, void* g_logits, void* stream) {
  if (T == 0) return 0;
  if (!logits || !g_logits || (((uintptr_t)logits | (uintptr_t)g_logits) & 15) || (!sigmoid && !lse) ||
      ((uintptr_t)lse & 3) || !ids || ((uintptr_t)ids & (ids_are_i64 ? 7 : 3)) ||
      (((uintptr_t)g_weights | (uintptr_t)g_lse | (uintptr_t)g_prob_sum) & 3))
    return MP4X_E_BADARG;
  const GateShape s = gate_shape(dtype, T, E);
  hipStream_t st = (hipStream_t)stream;
  return with_gate_dtype(dtype, [&](auto dtc) {
    constexpr int DT = decltype(dtc)::value;
    return with_gate_nv<DT>(s.NV, [&](auto nvc) {
      constexpr int NV = decltype(nvc)::value;
      const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(s.nblk), dim3(kBlock), 0, st, logits, lse, ids, ids_are_i64, T, E, K, s.G, s.lgG,
                           s.vec, renormalize != 0, scale, g_weights, g_lse, g_prob_sum, g_logits);
      };
      if (sigmoid) launch(k_moe_gate_bwd<DT, NV, true>);
      else launch(k_moe_gate_bwd<DT, NV, false>);
      return (int)hipGetLastError();
    });
  });
}

}  // namespace mp4x

using namespace mp4x;

extern "C" size_t mp4x_moe_gate_scratch_bytes(int dtype, int64_t T, int E) {
  if (gate_dtype_ok(dtype) || E < 1 || E > kGateMaxE || T < 0) return 0;
  const GateShape s = gate_shape(dtype, T, E);
  return gate_align((size_t)s.nblk * E * sizeof(float)) + gate_align((size_t)s.nblk * E * sizeof(int32_t));
}

extern "C" int mp4x_moe_gate_topk(int dtype, const void* logits, int64_t T, int E, int K, int renormalize,
                                  float* weights, void* ids, int ids_are_i64, float* lse, float* prob_sum,
                                  int64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
  if (int e = gate_args_ok(dtype, T, E, K)) return e;
  const GateShape s = gate_shape(dtype, T, E);
  hipStream_t st = (hipStream_t)stream;
  return gate_forward(dtype, s, logits, T, E, weights, ids, ids_are_i64, lse && !((uintptr_t)lse & 3), prob_sum, counts,
                      scratch, scratch_bytes, st, [&](auto dtc, auto nvc, auto statsc, size_t lds, float* psum_part,
                                                      int32_t* cnt_part) {
    hipLaunchKernelGGL((k_moe_gate_fwd<decltype(dtc)::value, decltype(nvc)::value, decltype(statsc)::value>), dim3(s.nblk),
                       dim3(kBlock), lds, st, logits, T, E, K, s.G, s.lgG, s.vec, renormalize != 0, weights, ids, ids_are_i64,
                       lse, psum_part, cnt_part);
  });
}

extern "C" int mp4x_moe_gate_backward(int dtype, const void* logits, const float* lse, const void* ids, int ids_are_i64,
                                      int64_t T, int E, int K, int renormalize, const float* g_weights,
                                      const float* g_lse, const float* g_prob_sum, void* g_logits, void* stream) {
  if (int e = gate_args_ok(dtype, T, E, K)) return e;
  return gate_backward(dtype, logits, lse, ids, ids_are_i64, T, E, K, 0, renormalize, 1.0f, g_weights, g_lse, g_prob_sum,
                       g_logits, stream);
}
