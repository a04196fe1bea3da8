// Shared device helpers for the mp4x CDNA4 kernels (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mp4x/ops.h"

namespace mp4x {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Device-side bounds checks of the debug build (tools/build_native.py --debug): report and trap
// the wave, so a bad index fails at its source instead of as a later memory fault.
#ifdef MP4X_DEBUG
#define MP4X_DASSERT(cond)                                                                     \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      printf("mp4x device assert failed: %s (%s:%d) block %d thread %d\n", #cond, __FILE__,    \
             __LINE__, (int)blockIdx.x, (int)threadIdx.x);                                     \
      __builtin_trap();                                                                        \
    }                                                                                          \
  } while (0)
#else
#define MP4X_DASSERT(cond) ((void)0)
#endif

constexpr int kBlock = 256;          // 4 wave64 per workgroup

// Global wave index of a kBlock-thread workgroup, made provably wave-uniform
// (readfirstlane): everything derived from it (block indices, mask / offset loads) then
// lives in SGPRs and is fetched with scalar loads instead of 64 copies in VGPRs.
__device__ __forceinline__ int64_t wave_id() {
  return (int64_t)blockIdx.x * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}
constexpr int kMaxGrid = 256 * 8;    // 256 CUs x 8 resident blocks: grid-stride beyond this

inline int grid_for(int64_t work_items, int per_thread = 1) {
  int64_t per_block = (int64_t)kBlock * per_thread;
  int64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > kMaxGrid) g = kMaxGrid;
  return (int)g;
}

// ---------------------------------------------------------------- 16-bit float helpers
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                          // round to nearest even
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float f16_to_f32(uint16_t h) {
  _Float16 x;
  __builtin_memcpy(&x, &h, 2);
  return (float)x;
}
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
  // The f32 value is pinned in a register first.  Left to itself the compiler fuses a product and
  // this conversion into v_fma_mixlo_f16 a, b, +0, and (-0) + (+0) = +0 loses the sign of a zero
  // product (f16 PROD and scale returned +0 for -0).
  asm("" : "+v"(f));
  _Float16 x = (_Float16)f;
  uint16_t h;
  __builtin_memcpy(&h, &x, 2);
  return h;
}

// ---------------------------------------------------------------- element traits
// Storage type S, accumulator type A, conversions.
template <int DT> struct Elem;
template <> struct Elem<MP4X_F64> { using S = double; using A = double;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_F32> { using S = float; using A = float;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_I64> { using S = int64_t; using A = int64_t;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_I32> { using S = int32_t; using A = int32_t;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_I16> { using S = int16_t; using A = int16_t;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_I8> { using S = int8_t; using A = int8_t;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_U8> { using S = uint8_t; using A = uint8_t;
  static __device__ A load(S s) { return s; } static __device__ S store(A a) { return a; } };
template <> struct Elem<MP4X_BF16> { using S = uint16_t; using A = float;
  static __device__ A load(S s) { return bf16_to_f32(s); } static __device__ S store(A a) { return f32_to_bf16(a); } };
template <> struct Elem<MP4X_F16> { using S = uint16_t; using A = float;
  static __device__ A load(S s) { return f16_to_f32(s); } static __device__ S store(A a) { return f32_to_f16(a); } };

template <int DT> constexpr bool is_float_dt() {
  return DT == MP4X_F64 || DT == MP4X_F32 || DT == MP4X_BF16 || DT == MP4X_F16;
}

// Which (dtype, op) pairs exist (mirrors the reference operator table + 16-bit floats).
template <int DT, int OP> constexpr bool op_valid() {
  if (OP == MP4X_SUM || OP == MP4X_MAX || OP == MP4X_MIN || OP == MP4X_PROD || OP == MP4X_FIRST) return true;
  if (OP == MP4X_BAND || OP == MP4X_BOR || OP == MP4X_BXOR) return !is_float_dt<DT>();
  if (OP == MP4X_FMAXLOC || OP == MP4X_FMINLOC) return DT == MP4X_F64;
  if (OP == MP4X_IMAXLOC || OP == MP4X_IMINLOC) return DT == MP4X_I64;
  return false;
}

template <typename T> struct Unsigned { using U = T; };
template <> struct Unsigned<int64_t> { using U = uint64_t; };
template <> struct Unsigned<int32_t> { using U = uint32_t; };
template <> struct Unsigned<int16_t> { using U = uint16_t; };
template <> struct Unsigned<int8_t> { using U = uint8_t; };

// combine(a, b): `a` is the accumulated (local / earlier) value, `b` the incoming one —
// the argument order of the reference's fused recv+reduce (DoubleOperand.java:196).
template <int DT, int OP>
__device__ __forceinline__ typename Elem<DT>::A combine(typename Elem<DT>::A a, typename Elem<DT>::A b) {
  using A = typename Elem<DT>::A;
  if constexpr (OP == MP4X_FIRST) {
    (void)b;
    return a;
  } else if constexpr (OP == MP4X_SUM) {
    if constexpr (is_float_dt<DT>()) return a + b;
    else { using U = typename Unsigned<A>::U; return (A)((U)a + (U)b); }
  } else if constexpr (OP == MP4X_PROD) {
    if constexpr (is_float_dt<DT>()) return a * b;
    else { using U = typename Unsigned<A>::U; return (A)((U)a * (U)b); }
  } else if constexpr (OP == MP4X_MAX) {
    if constexpr (is_float_dt<DT>()) return (a != a) ? a : ((b != b) ? b : (a >= b ? a : b));  // Java Math.max NaN rule
    else return a >= b ? a : b;
  } else if constexpr (OP == MP4X_MIN) {
    if constexpr (is_float_dt<DT>()) return (a != a) ? a : ((b != b) ? b : (a <= b ? a : b));
    else return a <= b ? a : b;
  } else if constexpr (OP == MP4X_BAND) {
    return a & b;
  } else if constexpr (OP == MP4X_BOR) {
    return a | b;
  } else if constexpr (OP == MP4X_BXOR) {
    return a ^ b;
  } else if constexpr (OP == MP4X_FMAXLOC || OP == MP4X_FMINLOC) {
    uint64_t ua, ub;
    __builtin_memcpy(&ua, &a, 8);
    __builtin_memcpy(&ub, &b, 8);
    float va = __uint_as_float((uint32_t)(ua >> 32)), vb = __uint_as_float((uint32_t)(ub >> 32));
    bool keep = (OP == MP4X_FMAXLOC) ? (va >= vb) : (va <= vb);   // ties keep the first argument
    return keep ? a : b;
  } else {  // IMAXLOC / IMINLOC on int64 words
    int32_t va = (int32_t)((uint64_t)a >> 32), vb = (int32_t)((uint64_t)b >> 32);
    bool keep = (OP == MP4X_IMAXLOC) ? (va >= vb) : (va <= vb);
    return keep ? a : b;
  }
}

// ---------------------------------------------------------------- 16-byte vectors of elements
// A packed value V (a 16-byte u32x4, or one storage element S) <-> its W accumulators.
template <int DT, typename V, int W>
__device__ __forceinline__ void unpack(const V& v, typename Elem<DT>::A (&a)[W]) {
  using E = Elem<DT>;
  typename E::S s[W];
  static_assert(sizeof(s) == sizeof(V), "W elements fill V");
  __builtin_memcpy(s, &v, sizeof(V));
#pragma unroll
  for (int j = 0; j < W; ++j) a[j] = E::load(s[j]);
}
template <int DT, typename V, int W>
__device__ __forceinline__ V pack(const typename Elem<DT>::A (&a)[W]) {
  using E = Elem<DT>;
  typename E::S s[W];
  static_assert(sizeof(s) == sizeof(V), "W elements fill V");
#pragma unroll
  for (int j = 0; j < W; ++j) s[j] = E::store(a[j]);
  V v;
  __builtin_memcpy(&v, s, sizeof(V));
  return v;
}

// acc[j] = combine(acc[j], element j of v): one more packed value folded into the accumulators
// (element by element: convert, combine — the order the kernels were tuned with).
template <int DT, int OP, typename V, int W>
__device__ __forceinline__ void fold_in(typename Elem<DT>::A (&acc)[W], const V& v) {
  using E = Elem<DT>;
  typename E::S s[W];
  static_assert(sizeof(s) == sizeof(V), "W elements fill V");
  __builtin_memcpy(s, &v, sizeof(V));
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = combine<DT, OP>(acc[j], E::load(s[j]));
}

// Combine of NR 16-byte vectors (rank order: r[0] first, deterministic), then the optional
// fused scale (float dtypes, a wave-uniform branch; 1.0 = plain reduction).  The fold of K1 and of
// every IPC kernel.  It stays one body, not unpack + fold_in + pack: written through them the
// compiler orders and allocates the IPC kernels differently (the same arithmetic), and their
// register budgets are part of the library (mp4x/_native/ipc_kernel_resources.json).
template <int DT, int OP, int NR>
__device__ __forceinline__ u32x4 fold_vec(const u32x4 (&r)[NR], float scale = 1.0f) {
  using E = Elem<DT>;
  using S = typename E::S;
  using A = typename E::A;
  constexpr int W = 16 / sizeof(S);
  S s[W];
  __builtin_memcpy(s, &r[0], 16);
  A acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = E::load(s[j]);
#pragma unroll
  for (int k = 1; k < NR; ++k) {
    S x[W];
    __builtin_memcpy(x, &r[k], 16);
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = combine<DT, OP>(acc[j], E::load(x[j]));
  }
  if constexpr (is_float_dt<DT>()) {
    if (scale != 1.0f) {
#pragma unroll
      for (int j = 0; j < W; ++j) acc[j] = acc[j] * (A)scale;
    }
  }
#pragma unroll
  for (int j = 0; j < W; ++j) s[j] = E::store(acc[j]);
  u32x4 o;
  __builtin_memcpy(&o, s, 16);
  return o;
}

// out[i] = the combine of element i of NIN inputs, in input order (scalar tails, unaligned operands).
template <int DT, int OP, int NIN>
__device__ __forceinline__ void fold_elem(void* out, const void* const (&ins)[NIN], int64_t i) {
  using E = Elem<DT>;
  using S = typename E::S;
  typename E::A acc = E::load(reinterpret_cast<const S*>(ins[0])[i]);
#pragma unroll
  for (int k = 1; k < NIN; ++k) acc = combine<DT, OP>(acc, E::load(reinterpret_cast<const S*>(ins[k])[i]));
  reinterpret_cast<S*>(out)[i] = E::store(acc);
}

// ---------------------------------------------------------------- host-side dispatch
// Every runtime (dtype, op) pair becomes template arguments here and nowhere else: a new dtype is
// a case of with_dtype (and an Elem), a new operator an entry of the op lists (and of op_valid /
// combine).
template <int V> using IntC = std::integral_constant<int, V>;

// f(IntC<DT>{}) for a runtime dtype code; `unknown` for a code outside the table.
template <typename F> inline int with_dtype(int dtype, F&& f, int unknown = MP4X_E_UNSUPPORTED) {
  switch (dtype) {
    case MP4X_F64: return f(IntC<MP4X_F64>{});
    case MP4X_F32: return f(IntC<MP4X_F32>{});
    case MP4X_I64: return f(IntC<MP4X_I64>{});
    case MP4X_I32: return f(IntC<MP4X_I32>{});
    case MP4X_I16: return f(IntC<MP4X_I16>{});
    case MP4X_I8: return f(IntC<MP4X_I8>{});
    case MP4X_BF16: return f(IntC<MP4X_BF16>{});
    case MP4X_F16: return f(IntC<MP4X_F16>{});
    case MP4X_U8: return f(IntC<MP4X_U8>{});
    default: return unknown;
  }
}

// The operator lists of the kernel families.
template <int... OPS> struct OpList {};
// the reference's operator table (MP4X_FIRST is a sparse-merge rule, not a collective operator):
// K1 and the IPC runtime-op kernels
using TableOps = OpList<MP4X_SUM, MP4X_MAX, MP4X_MIN, MP4X_PROD, MP4X_BAND, MP4X_BOR, MP4X_BXOR, MP4X_FMAXLOC,
                        MP4X_FMINLOC, MP4X_IMAXLOC, MP4X_IMINLOC>;
// row reductions of the hash / dense reduce-by-key ...
using RowOps = OpList<MP4X_SUM, MP4X_MAX, MP4X_MIN, MP4X_PROD, MP4X_BAND, MP4X_BOR, MP4X_BXOR>;
// ... and of the segmented reduce, which also serves the FIRST rule (K8)
using RowOpsFirst = OpList<MP4X_SUM, MP4X_MAX, MP4X_MIN, MP4X_PROD, MP4X_BAND, MP4X_BOR, MP4X_BXOR, MP4X_FIRST>;

// f(IntC<OP>{}) for a runtime op code of the list; MP4X_E_UNSUPPORTED for a listed op that is no
// operator of DT (op_valid), `unlisted` for a code outside the list.
template <int DT, int... OPS, typename F> inline int with_op_of(OpList<OPS...>, int op, int unlisted, F&& f) {
  int rc = unlisted;
  auto on = [&](auto opc) {
    constexpr int OP = decltype(opc)::value;
    if (op != OP) return false;
    if constexpr (op_valid<DT, OP>()) rc = f(opc);
    else rc = MP4X_E_UNSUPPORTED;
    return true;
  };
  (void)(on(IntC<OPS>{}) || ...);
  return rc;
}

// 0 when `op` is in the list and an operator of `dtype`, else MP4X_E_UNSUPPORTED.
template <typename Ops> inline int pair_supported(Ops ops, int dtype, int op) {
  return with_dtype(dtype, [&](auto dtc) {
    return with_op_of<decltype(dtc)::value>(ops, op, MP4X_E_UNSUPPORTED, [](auto) { return 0; });
  });
}

// f(IntC<N>{}) for a count LO..8 (K1's fan-in, the IPC kernels' rank count), else MP4X_E_BADARG.
template <int LO, typename F> inline int with_count(int n, F&& f) {
  switch (n) {
    case 1:
      if constexpr (LO <= 1) return f(IntC<1>{});
      return MP4X_E_BADARG;
    case 2: return f(IntC<2>{});
    case 3: return f(IntC<3>{});
    case 4: return f(IntC<4>{});
    case 5: return f(IntC<5>{});
    case 6: return f(IntC<6>{});
    case 7: return f(IntC<7>{});
    case 8: return f(IntC<8>{});
    default: return MP4X_E_BADARG;
  }
}

// Bytes per element of a dtype code (0: unknown), and whether it is a float dtype.
inline int elem_size(int dtype) {
  return with_dtype(dtype, [](auto dtc) { return (int)sizeof(typename Elem<decltype(dtc)::value>::S); }, 0);
}
inline bool float_dtype(int dtype) {
  return with_dtype(dtype, [](auto dtc) { return (int)is_float_dt<decltype(dtc)::value>(); }, 0) != 0;
}

}  // namespace mp4x
