// K13 — the group-limited, bias-corrected router gate (gfx950): K10's lane-group layout with a
// sigmoid or softmax score, a per-expert selection bias, a first selection of Kg of the Gr expert
// groups and a scaling factor on the gate weights.
//
// The layout is K10's (moe_gate.hip): a token's row over a lane group of G lanes, NV vectors per
// lane in registers, lane `sub` owns the columns (sub + v * G) * W + j.  Per token:
//
//   score      softmax: m = the row maximum (a __shfl_xor tree over the keys), sum and p as K10;
//              sigmoid: s = 1 / (1 + exp(-l)).  c = s + bias (one rounding) or s; -inf where l = -inf.
//   groups     for every group g < Gr (a loop bound from the launch arguments) a lane folds the keys
//              of c of its columns in g into a (largest, second) pair, a tree joins the pairs (max
//              and min of keys: exact, symmetric, so every lane holds the same bits and the result
//              does not depend on G); the group score is largest + second in one f32 addition, or
//              the largest alone when the second is -inf.  Lane g mod G keeps the score's key in
//              slot g / G (at most 16 slots).  Kg rounds of K10's argmax over (key, 2^32-1 - group)
//              pick the groups into a 32-bit mask.
//   ids        the live bits of columns outside the chosen groups are cleared, then K10's K rounds:
//              on the keys of the logits without a bias (K10's order for any bits), of c with one.
//   weights    q_k = the score of column ids_k, from one more (cached) load of that logit: the same
//              expression on the same bits as the score pass; / S (k order) and * scale.
//   statistics K10's: lane partials over the wave's tokens, LDS in (wave, group) order, per-block
//              partials to scratch, then k_moe_gate_stats.
//
// Only this forward kernel lives here; it stays apart from K10's, which scores only its K chosen
// columns and is the faster for it.  The backward is K10's k_moe_gate_bwd (moe_gate.hip, behind
// gate_backward) with the scale and, as a template argument, the sigmoid score:
// d_j = sigmoid(l_j) * sigmoid(-l_j).
// No floating-point atomics and no global atomics: every result is identical run to run.
#include <math.h>

#include "moe_gate_common.hpp"

namespace mp4x {

constexpr int kGateMaxGroups = 32;
constexpr int kGateGroupSlots = 16;   // group scores a lane keeps: ceil(Gr / G) <= 16 for every shape

template <int DT, int NV, bool STATS>
__global__ __launch_bounds__(kBlock) void k_moe_gate_group_fwd(
    const void* __restrict__ logits, const float* __restrict__ bias, int64_t T, int E, int K, int Gr, int Kg, int n,
    int sigmoid, int G, int lgG, int vec, int renorm, float scale, float* __restrict__ weights, void* __restrict__ ids,
    int ids_are_i64, int32_t* __restrict__ group_ids, float* __restrict__ lse, float* __restrict__ psum_part,
    int32_t* __restrict__ cnt_part) {
  using S = typename Elem<DT>::S;
  constexpr int W = 16 / sizeof(S);
  constexpr int LGW = W == 4 ? 2 : 3;
  constexpr int VPL = NV * W;
  static_assert(VPL <= 32, "the alive mask is 32 bits");
  extern __shared__ __attribute__((aligned(16))) char gate_group_smem[];
  float* lp = reinterpret_cast<float*>(gate_group_smem);                         // [4 * R][G * VPL] (STATS)
  int32_t* lh = reinterpret_cast<int32_t*>(gate_group_smem + (size_t)kBlock * VPL * sizeof(float));   // [E]
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = lane >> lgG, sub = lane & (G - 1), R = 64 >> lgG;
  const int64_t wave = wave_id();
  const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
  const uint32_t kNegInf = gate_key(-INFINITY);

  // what a lane's columns are does not depend on the token: in-range bits, the group of every
  // column (a byte each; 0xff past E) and its bias
  uint32_t inmask = 0;
  uint32_t gpack[VPL / 4];
  float bc[VPL];
#pragma unroll
  for (int i = 0; i < VPL / 4; ++i) gpack[i] = 0;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int col = (sub + (i / W) * G) * W + (i % W);
    const bool in = col < E;
    if (in) inmask |= 1u << i;
    const uint32_t g = in ? (uint32_t)col / (uint32_t)n : 0xffu;
    gpack[i / 4] |= g << ((i % 4) * 8);
    bc[i] = (bias && in) ? bias[col] : 0.0f;
  }
  const int nslot = (Gr + G - 1) >> lgG;            // <= kGateGroupSlots

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
    const int64_t tt = valid ? t : 0;
    float x[VPL];
    gate_load_row<DT, NV>(logits, t, E, G, sub, vec != 0, valid, 0.0f, x);

    // ---- the score: m and sum of the softmax as K10 has them
    float m = 0.0f, sum = 1.0f;
    if (!sigmoid) {
      uint32_t mk = 0;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const uint32_t k = ((inmask >> i) & 1u) ? gate_key(x[i]) : 0u;
        mk = k > mk ? k : mk;
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)mk, off);
        mk = o > mk ? o : mk;
      }
      m = gate_unkey(mk);
      float part = 0.0f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) part += ((inmask >> i) & 1u) ? expf(x[i] - m) : 0.0f;
      for (int off = G >> 1; off >= 1; off >>= 1) part += __shfl_xor(part, off);
      sum = part;
    }
    // the key of the selection score c of every column; -inf for a masked column and past E
    uint32_t ck[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const float s = sigmoid ? gate_sigmoid(x[i]) : expf(x[i] - m) / sum;
      float c = bias ? s + bc[i] : s;
      if (x[i] == -INFINITY) c = -INFINITY;
      ck[i] = ((inmask >> i) & 1u) ? gate_key(c) : kNegInf;
    }

    // ---- the group scores: slot r of lane `sub` holds the key of group r * G + sub
    uint32_t gk[kGateGroupSlots];
#pragma unroll
    for (int r = 0; r < kGateGroupSlots; ++r) gk[r] = 0;
    for (int g = 0; g < Gr; ++g) {
      uint32_t t1 = kNegInf, t2 = kNegInf;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const uint32_t gi = (gpack[i / 4] >> ((i % 4) * 8)) & 0xffu;
        const uint32_t k = gi == (uint32_t)g ? ck[i] : kNegInf;
        const uint32_t lo = k < t1 ? k : t1;
        t1 = k > t1 ? k : t1;
        t2 = lo > t2 ? lo : t2;
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)t1, off);
        const uint32_t o2 = (uint32_t)__shfl_xor((int)t2, off);
        const uint32_t lo = o1 < t1 ? o1 : t1;
        const uint32_t hi2 = o2 > t2 ? o2 : t2;
        t1 = o1 > t1 ? o1 : t1;
        t2 = lo > hi2 ? lo : hi2;
      }
      const float a = gate_unkey(t1);
      const uint32_t sk = gate_key(t2 == kNegInf ? a : a + gate_unkey(t2));
      const bool mine = sub == (g & (G - 1));
#pragma unroll
      for (int r = 0; r < kGateGroupSlots; ++r) {
        if (r >= nslot) continue;                     // uniform: most shapes use one slot
        gk[r] = (mine && r == (g >> lgG)) ? sk : gk[r];
      }
    }

    // ---- Kg rounds over the group scores: greater key, or equal key and smaller group
    uint32_t galive = 0, chosen = 0;
#pragma unroll
    for (int r = 0; r < kGateGroupSlots; ++r)
      if (r < nslot && r * G + sub < Gr) galive |= 1u << r;
    for (int kk = 0; kk < Kg; ++kk) {
      uint64_t best = 0;
#pragma unroll
      for (int r = 0; r < kGateGroupSlots; ++r) {
        if (r >= nslot) continue;
        const uint64_t c = ((galive >> r) & 1u) ? (((uint64_t)gk[r] << 32) | (0xffffffffu - (uint32_t)(r * G + sub))) : 0;
        best = c > best ? c : best;
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint64_t o = gate_shfl_xor(best, off);
        best = o > best ? o : best;
      }
      // Kg <= Gr live groups and one retired per round: a live pair always wins; the clamp holds
      // the group inside [0, Gr) whatever happens
      int g = (int)(0xffffffffu - (uint32_t)best);
      MP4X_DASSERT(g >= 0 && g < Gr);
      g = g < 0 ? 0 : (g >= Gr ? Gr - 1 : g);
      if (sub == (g & (G - 1))) galive &= ~(1u << (g >> lgG));
      chosen |= 1u << g;
      if (valid && group_ids && sub == 0) group_ids[t * Kg + kk] = g;
    }

    // ---- the K rounds inside the chosen groups
    uint32_t alive = 0;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const uint32_t gi = (gpack[i / 4] >> ((i % 4) * 8)) & 0x1fu;
      if (((inmask >> i) & 1u) && ((chosen >> gi) & 1u)) alive |= 1u << i;
    }
    int idk[kGateMaxK];
#pragma unroll
    for (int k = 0; k < kGateMaxK; ++k) {
      idk[k] = 0;
      if (k >= K) continue;
      uint64_t best = 0;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const uint32_t col = (uint32_t)((sub + (i / W) * G) * W + (i % W));
        const uint32_t key = bias ? ck[i] : gate_key(x[i]);
        const uint64_t c = ((alive >> i) & 1u) ? (((uint64_t)key << 32) | (0xffffffffu - col)) : 0;
        best = c > best ? c : best;
      }
      for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint64_t o = gate_shfl_xor(best, off);
        best = o > best ? o : best;
      }
      // K <= Kg * n live columns and one retired per round: a live pair always wins.  The clamp
      // holds the id inside [0, E) whatever happens.
      int col = (int)(0xffffffffu - (uint32_t)best);
      MP4X_DASSERT(col >= 0 && col < E);
      col = col < 0 ? 0 : (col >= E ? E - 1 : col);
      const int vi = col >> LGW;
      if (sub == (vi & (G - 1))) alive &= ~(1u << (((vi >> lgG) << LGW) | (col & (W - 1))));
      idk[k] = col;
    }

    // ---- the gate weights: the score of the chosen columns, not c
    float q[kGateMaxK];
    float ssum = 0.0f;
#pragma unroll
    for (int k = 0; k < kGateMaxK; ++k) {
      q[k] = 0.0f;
      if (k >= K) continue;
      const float l = Elem<DT>::load(reinterpret_cast<const S*>(logits)[tt * E + idk[k]]);
      q[k] = sigmoid ? gate_sigmoid(l) : expf(l - m) / sum;
      ssum += q[k];
    }
    if (valid) {
      if (lse && !sigmoid && sub == 0) lse[t] = m + logf(sum);
#pragma unroll
      for (int k = 0; k < kGateMaxK; ++k) {
        if (k >= K) continue;
        if ((k & (G - 1)) == sub) {
          const int64_t a = t * K + k;
          weights[a] = (renorm ? q[k] / ssum : q[k]) * scale;
          if (ids_are_i64) reinterpret_cast<int64_t*>(ids)[a] = idk[k];
          else reinterpret_cast<int32_t*>(ids)[a] = idk[k];
          if constexpr (STATS) atomicAdd(&lh[idk[k]], 1);
        }
      }
      if constexpr (STATS) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const float s = sigmoid ? gate_sigmoid(x[i]) : expf(x[i] - m) / sum;
          acc[i] += ((inmask >> i) & 1u) ? s : 0.0f;
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
      for (int qq = 0; qq < 4 * R; ++qq) a += lp[(size_t)qq * stride + e];      // (wave, group) order
      psum_part[(int64_t)blockIdx.x * E + e] = a;
      cnt_part[(int64_t)blockIdx.x * E + e] = lh[e];
    }
  }
}

}  // namespace mp4x

using namespace mp4x;

namespace {
int gate_group_args_ok(int dtype, int64_t T, int E, int K, int score, int Gr, int Kg, float scale) {
  if (int e = gate_dtype_ok(dtype)) return e;
  if (score != 0 && score != 1) return MP4X_E_UNSUPPORTED;
  if (int e = gate_args_ok(dtype, T, E, K)) return e;
  if (Gr < 1 || Gr > kGateMaxGroups || E % Gr || Kg < 1 || Kg > Gr || K > (int64_t)Kg * (E / Gr)) return MP4X_E_BADARG;
  if (!(scale > 0.0f) || !std::isfinite(scale)) return MP4X_E_BADARG;
  return 0;
}
}  // namespace

extern "C" size_t mp4x_moe_gate_group_scratch_bytes(int dtype, int64_t T, int E) {
  return mp4x_moe_gate_scratch_bytes(dtype, T, E);
}

extern "C" int mp4x_moe_gate_group_topk(int dtype, const void* logits, const float* bias, int64_t T, int E, int K,
                                        int n_group, int topk_group, int score, int renormalize, float scale,
                                        float* weights, void* ids, int ids_are_i64, int32_t* group_ids, float* lse,
                                        float* prob_sum, int64_t* counts, void* scratch, size_t scratch_bytes,
                                        void* stream) {
  if (int e = gate_group_args_ok(dtype, T, E, K, score, n_group, topk_group, scale)) return e;
  if (((uintptr_t)bias | (uintptr_t)group_ids | (uintptr_t)lse) & 3) return MP4X_E_BADARG;
  const GateShape s = gate_shape(dtype, T, E);
  const bool others_ok = (score != 0 || lse) && ((n_group + s.G - 1) >> s.lgG) <= kGateGroupSlots;   // every shape has the slots
  hipStream_t st = (hipStream_t)stream;
  const int n = E / n_group;
  return gate_forward(dtype, s, logits, T, E, weights, ids, ids_are_i64, others_ok, prob_sum, counts, scratch, scratch_bytes,
                      st, [&](auto dtc, auto nvc, auto statsc, size_t lds, float* psum_part, int32_t* cnt_part) {
    hipLaunchKernelGGL((k_moe_gate_group_fwd<decltype(dtc)::value, decltype(nvc)::value, decltype(statsc)::value>),
                       dim3(s.nblk), dim3(kBlock), lds, st, logits, bias, T, E, K, n_group, topk_group, n, score, s.G, s.lgG,
                       s.vec, renormalize != 0, scale, weights, ids, ids_are_i64, group_ids, lse, psum_part, cnt_part);
  });
}

extern "C" int mp4x_moe_gate_group_backward(int dtype, const void* logits, const float* lse, const void* ids,
                                            int ids_are_i64, int64_t T, int E, int K, int score, int renormalize,
                                            float scale, const float* g_weights, const float* g_lse,
                                            const float* g_prob_sum, void* g_logits, void* stream) {
  if (int e = gate_group_args_ok(dtype, T, E, K, score, 1, 1, scale)) return e;
  return gate_backward(dtype, logits, lse, ids, ids_are_i64, T, E, K, score, renormalize, scale, g_weights, g_lse,
                       g_prob_sum, g_logits, stream);
}
