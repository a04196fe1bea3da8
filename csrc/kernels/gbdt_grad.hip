// K21 — GBDT losses on the GPU: margins -> quantised (g, h) pairs with no float gradient in memory (gfx950).
//
// The rules (squared, logistic, softmax over C classes; an exp written as a fixed sequence of float64
// operations) are gbdt_loss_map.hpp's, the same code on the host; this file is how rows are spread over
// lanes.  Margins are class-major, pred f64[C, n] and gh int32[C, n, 2]: a lane owns rows, so every load of
// a class is coalesced and gh[c] is the tensor the K16 kernels take.
//
//   absmax    k_gbdt_grad_zero      top = 0 (a kernel, so a captured graph holds no memset node)
//             k_gbdt_grad_absmax    a block of 256 lanes serves 1024 consecutive rows, kRows = 4 a lane (row
//                                   tid + 256 j).  A lane opens its rows (softmax: the label, m and S), then per
//                                   class computes (g, h) of its four rows in registers and keeps the larger
//                                   key = bits & 0x7fffffff of each; one xor-shuffle reduce a class and
//                                   component in the wave, lane 0's result into the block's LDS table with a
//                                   32-bit integer max, and after the barrier one global integer atomicMax per
//                                   non-zero (class, component).  Four rows a lane amortise the shuffles.
//                                   Integer max has no order: top is a function of the input.  Nothing but
//                                   top is written
//   quantize  k_gbdt_grad_quantize  a lane owns the rows 2i, 2i + 1: per class it recomputes (g, h) of both,
//                                   applies K16's quantiser (gbdt_map::q) with the class's shifts read from
//                                   device memory (clamped to +-200) and writes the pair with one 16-byte
//                                   store.  Class c's pair stands at element c n + 2i: where that is odd (n
//                                   odd, c odd; wave-uniform) the 16-byte load and store become two 8-byte
//                                   ones.  The last row of an odd n takes the one-row tail form
//
// Softmax makes three passes over a row's C margins (the maximum, the sum, the outputs).  C is a run-time
// number up to 64, so e_c is not kept: the second and third pass read pred again, the same coalesced
// addresses from the same lanes, which the caches serve; e_c is computed twice.  Per row the quantise kernel
// reads 8 C + 8 bytes from memory and writes 8 C.
//
// No float atomics, no host synchronisation, no allocation, exact grids: recordable in a graph.  Compiled
// without the packed f32 instructions, like gbdt.hip.
#include "common.hpp"
#include "gbdt_loss_map.hpp"

namespace mp4x {

namespace gl = gbdt_loss;
namespace gm = gbdt_map;
static_assert(gl::kBlock == kBlock, "the loss kernels use the common block");

// What a lane keeps of a row between the classes.
template <int LOSS> struct GradRow {
  double y;
};
template <> struct GradRow<gl::kSoftmax> {
  double m, S;
  int64_t y;
};

template <int LOSS>
__device__ __forceinline__ GradRow<LOSS> grad_open(const double* __restrict__ pred, const void* __restrict__ y, int64_t n,
                                                   int C, int64_t r) {
  GradRow<LOSS> row;
  if constexpr (LOSS == gl::kSoftmax) {
    row.y = reinterpret_cast<const int64_t*>(y)[r];
    double m = pred[r];
    for (int c = 1; c < C; ++c) m = gl::max_step(m, pred[(int64_t)c * n + r]);
    double S = gl::soft_e(m, pred[r]);
    for (int c = 1; c < C; ++c) S = S + gl::soft_e(m, pred[(int64_t)c * n + r]);
    row.m = m;
    row.S = S;
  } else {
    row.y = reinterpret_cast<const double*>(y)[r];
  }
  return row;
}

// (g, h) of class c of an opened row, x its margin.
template <int LOSS> __device__ __forceinline__ gl::Pair grad_pair(const GradRow<LOSS>& row, double x, int c, int C) {
  if constexpr (LOSS == gl::kSquared) {
    return gl::squared(x, row.y);
  } else if constexpr (LOSS == gl::kLogistic) {
    return gl::logistic(x, row.y);
  } else {
    if (!gl::label_ok(row.y, C)) return gl::Pair{0.0f, 0.0f};
    return gl::soft_pair(gl::soft_e(row.m, x), row.S, row.y == (int64_t)c);
  }
}

__global__ __launch_bounds__(kBlock) void k_gbdt_grad_zero(uint32_t* __restrict__ top, int words) {
  if ((int)threadIdx.x < words) top[threadIdx.x] = 0;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  return v;
}

template <int LOSS>
__global__ __launch_bounds__(kBlock) void k_gbdt_grad_absmax(const double* __restrict__ pred, const void* __restrict__ y,
                                                             int64_t n, int C, uint32_t* __restrict__ top) {
  __shared__ uint32_t ltop[2 * gl::kMaxClasses];
  const int tid = threadIdx.x;
  if (tid < 2 * C) ltop[tid] = 0;                          // 2 C <= 128 < kBlock
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * (kBlock * gl::kRows) + tid;
  GradRow<LOSS> row[gl::kRows];
#pragma unroll
  for (int j = 0; j < gl::kRows; ++j) {
    const int64_t r = r0 + (int64_t)j * kBlock;
    if (r < n) row[j] = grad_open<LOSS>(pred, y, n, C, r);
  }
  for (int c = 0; c < C; ++c) {                            // every lane of the wave takes every trip: the shuffles are whole
    const double* pc = pred + (int64_t)c * n;
    uint32_t kg = 0, kh = 0;
#pragma unroll
    for (int j = 0; j < gl::kRows; ++j) {
      const int64_t r = r0 + (int64_t)j * kBlock;
      if (r < n) {
        const gl::Pair p = grad_pair<LOSS>(row[j], pc[r], c, C);
        const uint32_t a = gl::key(p.g), b = gl::key(p.h);
        kg = a > kg ? a : kg;
        kh = b > kh ? b : kh;
      }
    }
    kg = wave_max(kg);
    kh = wave_max(kh);
    if ((tid & 63) == 0) {
      if (kg) atomicMax(&ltop[2 * c], kg);
      if (kh) atomicMax(&ltop[2 * c + 1], kh);
    }
  }
  __syncthreads();
  if (tid < 2 * C) {
    const uint32_t v = ltop[tid];
    if (v) atomicMax(&top[tid], v);
  }
}

template <int LOSS>
__global__ __launch_bounds__(kBlock) void k_gbdt_grad_quantize(const double* __restrict__ pred, const void* __restrict__ y,
                                                               int64_t n, int C, const int32_t* __restrict__ sg,
                                                               const int32_t* __restrict__ sh, int32_t* __restrict__ gh) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 2;
  if (r >= n) return;
  if (r + 1 < n) {
    const GradRow<LOSS> ra = grad_open<LOSS>(pred, y, n, C, r), rb = grad_open<LOSS>(pred, y, n, C, r + 1);
    for (int c = 0; c < C; ++c) {
      const int64_t at = (int64_t)c * n + r;               // r is even: the parity of `at` is the wave's
      const int s_g = gl::shift(sg[c]), s_h = gl::shift(sh[c]);
      const bool whole = !(at & 1);
      double xa, xb;
      if (whole) {
        const double2 v = *reinterpret_cast<const double2*>(pred + at);
        xa = v.x;
        xb = v.y;
      } else {
        xa = pred[at];
        xb = pred[at + 1];
      }
      const gl::Pair pa = grad_pair<LOSS>(ra, xa, c, C), pb = grad_pair<LOSS>(rb, xb, c, C);
      int4 o;
      o.x = gm::q(pa.g, s_g);
      o.y = gm::q(pa.h, s_h);
      o.z = gm::q(pb.g, s_g);
      o.w = gm::q(pb.h, s_h);
      if (whole) {
        *reinterpret_cast<int4*>(gh + 2 * at) = o;
      } else {
        *reinterpret_cast<int2*>(gh + 2 * at) = make_int2(o.x, o.y);
        *reinterpret_cast<int2*>(gh + 2 * at + 2) = make_int2(o.z, o.w);
      }
    }
  } else {                                                 // the last row of an odd n
    const GradRow<LOSS> ra = grad_open<LOSS>(pred, y, n, C, r);
    for (int c = 0; c < C; ++c) {
      const int64_t at = (int64_t)c * n + r;
      const gl::Pair pa = grad_pair<LOSS>(ra, pred[at], c, C);
      *reinterpret_cast<int2*>(gh + 2 * at) = make_int2(gm::q(pa.g, gl::shift(sg[c])), gm::q(pa.h, gl::shift(sh[c])));
    }
  }
}

// f(IntC<LOSS>{}) for a loss code.
template <typename F> inline int with_loss(int loss, F&& f) {
  switch (loss) {
    case gl::kSquared: return f(IntC<gl::kSquared>{});
    case gl::kLogistic: return f(IntC<gl::kLogistic>{});
    case gl::kSoftmax: return f(IntC<gl::kSoftmax>{});
    default: return MP4X_E_BADARG;
  }
}

// The argument rule both calls share; `out` is top or gh.
inline int grad_args(const double* pred, const void* y, int64_t n, int C, int loss, const void* out, int out_align) {
  if (n < 0 || n >= gm::kMaxRows || C < 1 || C > gl::kMaxClasses || loss < gl::kSquared || loss > gl::kSoftmax ||
      (loss != gl::kSoftmax && C != 1))
    return MP4X_E_BADARG;
  if (n == 0) return 0;
  if (!pred || ((uintptr_t)pred & 15) || !y || ((uintptr_t)y & 7) || !out || ((uintptr_t)out & (out_align - 1)))
    return MP4X_E_BADARG;
  return 0;
}

}  // namespace mp4x

using namespace mp4x;

extern "C" int mp4x_gbdt_grad_absmax(const double* pred, const void* y, int64_t n, int C, int loss, float* top,
                                     void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (int e = grad_args(pred, y, n, C, loss, top, 4)) return e;
  if (!top || ((uintptr_t)top & 3)) return MP4X_E_BADARG;
  hipLaunchKernelGGL(k_gbdt_grad_zero, dim3(1), dim3(kBlock), 0, st, (uint32_t*)top, 2 * C);
  if (int e = (int)hipGetLastError()) return e;
  if (n == 0) return 0;
  const int64_t per = (int64_t)kBlock * gl::kRows, blocks = (n + per - 1) / per;   // n < 2^31: below 2^21 blocks
  return with_loss(loss, [&](auto lc) {
    hipLaunchKernelGGL(k_gbdt_grad_absmax<decltype(lc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0, st, pred, y, n, C,
                       (uint32_t*)top);
    return (int)hipGetLastError();
  });
}

extern "C" int mp4x_gbdt_grad_quantize(const double* pred, const void* y, int64_t n, int C, int loss, const int32_t* sg,
                                       const int32_t* sh, int32_t* gh, void* stream) {
  if (int e = grad_args(pred, y, n, C, loss, gh, 16)) return e;
  if (n == 0) return 0;
  if (!sg || ((uintptr_t)sg & 3) || !sh || ((uintptr_t)sh & 3)) return MP4X_E_BADARG;
  const int64_t blocks = (n + 2 * kBlock - 1) / (2 * kBlock);
  return with_loss(loss, [&](auto lc) {
    hipLaunchKernelGGL(k_gbdt_grad_quantize<decltype(lc)::value>, dim3((unsigned)blocks), dim3(kBlock), 0,
                       (hipStream_t)stream, pred, y, n, C, sg, sh, gh);
    return (int)hipGetLastError();
  });
}
