// The loss rules of the GBDT gradient kernels (K21, gbdt_grad.hip): margins -> (g, h) in float32, with an
// exp that is specified.  Plain C++ (no HIP types), the same code on the host and on the device; the
// torch form of the same operations is gbdt_grad_torch (mp4x/parallel/gbdt.py).  Every operation below is
// one IEEE float64 operation rounded once (no contraction: MP4X_LOSS_EXACT opens every body, and the
// statements are written one operation each), then one rounding to float32, so the host, the device and
// torch give the same bits.
//
// exp_neg(t) = exp(-t) for t in [0, 708]; a NaN t returns itself before any integer is formed:
//   k = rint(-t * kInvLn2)                       half to even; -1022 < k <= 0
//   r = (-t - k * kLn2Hi) - k * kLn2Lo            kLn2Hi ends in 21 zero bits and |k| < 2^10: the product is exact
//   p = Horner in r over 1 / 13! .. 1 / 0!         the Taylor polynomial of degree 13, |r| <= 0.35
//   exp_neg = p * 2^k                             2^k by its exponent bits, k + 1023 in [2, 1023]: normal
// About 1 ulp from expl over the range (tests/test_gbdt_loss_map_cpu.py holds 4).
//
// squared    g = f32(x - y), h = 1
// logistic   t = |x| > 708 ? 708 : |x| (a NaN passes), e = exp_neg(t), d = 1 + e; with a = 1 / d, b = e / d:
//            p = x >= 0 ? a : b, q = the other; g = f32(p - y), h = f32(p * q).  The clamp is invisible in
//            float32; a NaN x gives NaN g and h.
// softmax    m = the maximum of the row's C margins, NaN winning (max_step, in class order); t_c = m - x_c
//            clamped as above, e_c = exp_neg(t_c); S = e_0 + e_1 + .. in class order; p_c = e_c / S;
//            g_c = f32(p_c - [y == c]), h_c = f32(p_c * (1 - p_c)).  A row with a NaN or +inf margin is NaN
//            throughout (inf - inf); a label outside [0, C) makes all 2C outputs +0.
//
// key(bits) = bits & 0x7fffffff of a float32: its magnitude in an unsigned order where every NaN stands above
// infinity, the order torch.max propagates NaN in.  q(x, s) is K16's quantiser (gbdt_hist_map.hpp); a shift
// read from device memory is clamped to +-kMaxShift first (shift), so any bits are legal there.
#pragma once
#include <stdint.h>

#include "gbdt_hist_map.hpp"

#if defined(__clang__)
#define MP4X_LOSS_EXACT _Pragma("clang fp contract(off)")
#else
#define MP4X_LOSS_EXACT
#endif

namespace mp4x {
namespace gbdt_loss {

constexpr int kMaxClasses = 64;                  // C: the kernels' per-block key table is 2 * kMaxClasses words
constexpr int kSquared = 0, kLogistic = 1, kSoftmax = 2;
constexpr int kBlock = 256;
constexpr int kRows = 4;                         // rows a lane of the absmax kernel: one wave reduce a class serves 256
constexpr double kClamp = 708.0;
constexpr double kInvLn2 = 0x1.71547652b82fep+0;
constexpr double kLn2Hi = 0x1.62e42fee00000p-1;
constexpr double kLn2Lo = 0x1.a39ef35793c76p-33;

struct Pair {
  float g, h;
};

MP4X_GBDT_HD double from_bits(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
MP4X_GBDT_HD uint32_t key(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u & 0x7fffffffu;
}
MP4X_GBDT_HD float key_float(uint32_t k) {
  float x;
  __builtin_memcpy(&x, &k, 4);
  return x;
}

// One Horner step: two roundings.
MP4X_GBDT_HD double horner(double p, double r, double c) {
  MP4X_LOSS_EXACT
  const double pr = p * r;
  return pr + c;
}
// k of exp_neg, for t in [0, 708]: an integer in (-1022, 0].
MP4X_GBDT_HD double exp_k(double t) {
  MP4X_LOSS_EXACT
  const double x = -t;
  const double s = x * kInvLn2;
  return __builtin_rint(s);
}
MP4X_GBDT_HD double exp_neg(double t) {
  MP4X_LOSS_EXACT
  if (t != t) return t;
  const double x = -t;
  const double k = exp_k(t);
  const double hi = k * kLn2Hi;
  const double lo = k * kLn2Lo;
  const double r0 = x - hi;
  const double r = r0 - lo;
  double p = 0x1.6124613a86d09p-33;          // 1 / 13!; below 1 / 12! .. 1 / 0!, each the nearest float64
  p = horner(p, r, 0x1.1eed8eff8d898p-29);
  p = horner(p, r, 0x1.ae64567f544e4p-26);
  p = horner(p, r, 0x1.27e4fb7789f5cp-22);
  p = horner(p, r, 0x1.71de3a556c734p-19);
  p = horner(p, r, 0x1.a01a01a01a01ap-16);
  p = horner(p, r, 0x1.a01a01a01a01ap-13);
  p = horner(p, r, 0x1.6c16c16c16c17p-10);
  p = horner(p, r, 0x1.1111111111111p-7);
  p = horner(p, r, 0x1.5555555555555p-5);
  p = horner(p, r, 0x1.5555555555555p-3);
  p = horner(p, r, 0x1.0000000000000p-1);
  p = horner(p, r, 0x1.0000000000000p+0);
  p = horner(p, r, 0x1.0000000000000p+0);
  const double scale = from_bits((uint64_t)((int64_t)k + 1023) << 52);
  return p * scale;
}
// min(t, 708) that lets a NaN through.
MP4X_GBDT_HD double clamp_t(double t) { return t > kClamp ? kClamp : t; }

MP4X_GBDT_HD Pair squared(double x, double y) {
  MP4X_LOSS_EXACT
  const double d = x - y;
  return Pair{(float)d, 1.0f};
}

MP4X_GBDT_HD Pair logistic(double x, double y) {
  MP4X_LOSS_EXACT
  const double e = exp_neg(clamp_t(__builtin_fabs(x)));
  const double d = 1.0 + e;
  const double a = 1.0 / d;
  const double b = e / d;
  const bool up = x >= 0.0;
  const double p = up ? a : b, q = up ? b : a;
  const double g = p - y;
  const double h = p * q;
  return Pair{(float)g, (float)h};
}

// The running maximum of a row's margins, a NaN winning: m = max_step(m, x_c) for c = 1 .. C - 1 from m = x_0.
MP4X_GBDT_HD double max_step(double m, double x) { return m != m ? m : (x != x || x > m) ? x : m; }
MP4X_GBDT_HD double soft_e(double m, double x) {
  MP4X_LOSS_EXACT
  const double t = m - x;
  return exp_neg(clamp_t(t));
}
MP4X_GBDT_HD bool label_ok(int64_t y, int C) { return y >= 0 && y < (int64_t)C; }
// Class c of a row whose label is in range: e = soft_e(m, x_c), S the row's sum, hit = (y == c).
MP4X_GBDT_HD Pair soft_pair(double e, double S, bool hit) {
  MP4X_LOSS_EXACT
  const double p = e / S;
  const double g = p - (hit ? 1.0 : 0.0);
  const double u = 1.0 - p;
  const double h = p * u;
  return Pair{(float)g, (float)h};
}

MP4X_GBDT_HD int shift(int32_t s) {
  return s < -gbdt_map::kMaxShift ? -gbdt_map::kMaxShift : s > gbdt_map::kMaxShift ? gbdt_map::kMaxShift : s;
}

}  // namespace gbdt_loss
}  // namespace mp4x
