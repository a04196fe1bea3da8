// Stand-alone CPU test of the GBDT loss rules (gbdt_loss_map.hpp): exp_neg against expl within 4 ulp over the
// hostile margins of the Python tests and a seeded spread of [0, 708], every k inside (-1022, 0] and every
// exponent field of 2^k inside [2, 1023], the logistic and softmax pairs inside their ranges (p in [0, 1], h in
// [0, 1/4]), NaN and +inf rows NaN throughout, a label out of range +0 throughout, the shift clamp, and the
// quantiser of every pair inside +-kQMax.  Built by tests/test_gbdt_loss_map_cpu.py with
// -fsanitize=address,undefined: a NaN or out-of-range value turned into an integer is an error there.  Prints OK.
#include <cmath>
#include <cstdint>
#include <vector>

#include "gbdt_loss_map.hpp"
#include "test_map_common.hpp"

namespace gl = mp4x::gbdt_loss;
namespace gm = mp4x::gbdt_map;

static double ulps(double got, long double want) {
  int e;
  std::frexp((double)want, &e);
  const int low = e - 53 < -1074 ? -1074 : e - 53;            // the exponent of want's last place
  return (double)(std::fabs((long double)got - want) / std::ldexp(1.0L, low));
}

static void check_pair(gl::Pair p, double glo, double ghi, const char* what, double x) {
  CHECK(p.g >= glo && p.g <= ghi && p.h >= 0.0f && p.h <= 0.25f, "%s at %a: g %a h %a", what, x, p.g, p.h);
  for (int s : {-gm::kMaxShift, 0, 30, gm::kMaxShift}) {
    const int32_t a = gm::q(p.g, s), b = gm::q(p.h, s);
    CHECK(a >= -gm::kQMax && a <= gm::kQMax && b >= 0 && b <= gm::kQMax, "%s at %a shift %d", what, x, s);
  }
}

int main() {
  std::vector<double> xs = {0.0, 1e-320, 0.5, 36.7, 100.0, 708.0, 709.0, 800.0, 1e300, INFINITY};
  uint64_t state = 12345;
  for (int i = 0; i < 20000; ++i) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    xs.push_back((double)(state >> 11) * 0x1p-53 * (i % 2 ? 708.0 : 40.0));
  }
  double worst = 0.0;
  for (double x : xs) {
    const double t = gl::clamp_t(x);
    const double k = gl::exp_k(t);
    CHECK(k > -1022.0 && k <= 0.0 && k == std::rint(k), "k %a at %a", k, t);
    const int64_t field = (int64_t)k + 1023;
    CHECK(field >= 2 && field <= 1023, "exponent field %lld at %a", (long long)field, t);
    const double e = gl::exp_neg(t);
    const double u = ulps(e, expl(-(long double)t));
    worst = u > worst ? u : worst;
    CHECK(u <= 4.0 && e > 0.0 && e <= 1.0, "exp_neg(%a) = %a, %g ulp", t, e, u);
    for (double sx : {x, -x}) {
      check_pair(gl::logistic(sx, 0.0), 0.0, 1.0, "logistic", sx);
      check_pair(gl::logistic(sx, 1.0), -1.0, 0.0, "logistic", sx);
      const double row[3] = {sx, 0.25, -3.0};                 // softmax over (x, 1/4, -3), label 1
      double m = row[0];
      for (int c = 1; c < 3; ++c) m = gl::max_step(m, row[c]);
      double S = gl::soft_e(m, row[0]);
      for (int c = 1; c < 3; ++c) S = S + gl::soft_e(m, row[c]);
      const bool broken = sx == INFINITY;                     // +inf: NaN throughout
      CHECK(broken ? S != S : (S >= 1.0 && S <= 3.0), "S %a at %a", S, sx);
      for (int c = 0; c < 3; ++c) {
        const gl::Pair p = gl::soft_pair(gl::soft_e(m, row[c]), S, c == 1);
        if (broken) CHECK(p.g != p.g && p.h != p.h && gm::q(p.g, 30) == 0, "class %d of a +inf row", c);
        else check_pair(p, c == 1 ? -1.0 : 0.0, c == 1 ? 0.0 : 1.0, "softmax", sx);
      }
    }
  }
  const double nan = std::nan("");
  const gl::Pair p = gl::logistic(nan, 0.0);
  CHECK(p.g != p.g && p.h != p.h && gl::exp_neg(nan) != gl::exp_neg(nan) && gl::max_step(1.0, nan) != gl::max_step(nan, 1.0));
  CHECK(gl::logistic(-0.0, 0.0).g == 0.5f && gl::squared(1e300, 0.0).g == INFINITY && gl::squared(3.0, 1.0).h == 1.0f);
  CHECK(!gl::label_ok(-1, 3) && !gl::label_ok(3, 3) && gl::label_ok(2, 3) && !gl::label_ok(INT64_MIN, 64));
  CHECK(gl::shift(INT32_MIN) == -gm::kMaxShift && gl::shift(INT32_MAX) == gm::kMaxShift && gl::shift(-7) == -7);
  CHECK(gl::key(-INFINITY) == 0x7f800000u && gl::key((float)nan) > 0x7f800000u && gl::key(-0.0f) == 0u &&
        gl::key_float(gl::key(-2.5f)) == 2.5f);
  return map_test::report("OK %zu margins, exp_neg within %.2f ulp of expl\n", xs.size(), worst);
}
