// rgbl::po_sin / po_cos (csrc/poseopt_math.h) against the live libm's sin / cos (tests/test_pose_opt_math.py builds and runs this):
//   small   2^22 arguments evenly spaced over [0, 8] and their negatives: what SE3Quat::exp can see (theta = |omega| of an update)
//   wide    2^22 doubles evenly spaced in bit pattern over [1e-9, 2^20], the supported range
// Prints, per range and function, the largest difference in units of the libm result's last place, how many results differ
// at all and the largest absolute difference.  libm's sin / cos are themselves within 1 ulp of the true value, not correctly rounded.
// Built with -ffp-contract=off -fno-builtin.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../orb_slam3_rgbl_amd/csrc/poseopt_math.h"

static uint64_t bits(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }
static double from_bits(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }
static double ulps(double got, double want) {
  if (got == want) return 0.0;
  const double ulp = nextafter(fabs(want), INFINITY) - fabs(want);
  return fabs(got - want) / ulp;
}

struct Worst { double u = 0.0, at = 0.0, abs = 0.0; uint64_t differ = 0; };
static void take(Worst& w, double got, double want, double x) {
  const double u = ulps(got, want);
  if (u > 0.0) ++w.differ;
  if (fabs(got - want) > w.abs) w.abs = fabs(got - want);
  if (u > w.u) { w.u = u; w.at = x; }
}

int main() {
  const int N = 1 << 22;
  Worst s_small, c_small, s_wide, c_wide;
  for (int i = 0; i <= N; ++i) {
    for (int sign = -1; sign <= 1; sign += 2) {
      const double x = sign * 8.0 * i / N;
      take(s_small, rgbl::po_sin(x), sin(x), x);
      take(c_small, rgbl::po_cos(x), cos(x), x);
    }
  }
  const uint64_t lo = bits(1e-9), hi = bits(1048576.0);
  for (int i = 0; i <= N; ++i) {
    const double x = from_bits(lo + (uint64_t)((double)(hi - lo) * i / N));
    take(s_wide, rgbl::po_sin(x), sin(x), x);
    take(c_wide, rgbl::po_cos(x), cos(x), x);
  }
  printf("small sin max_ulp %.3f at %a differ %llu max_abs %.3e\n", s_small.u, s_small.at, (unsigned long long)s_small.differ, s_small.abs);
  printf("small cos max_ulp %.3f at %a differ %llu max_abs %.3e\n", c_small.u, c_small.at, (unsigned long long)c_small.differ, c_small.abs);
  printf("wide sin max_ulp %.3f at %a differ %llu max_abs %.3e\n", s_wide.u, s_wide.at, (unsigned long long)s_wide.differ, s_wide.abs);
  printf("wide cos max_ulp %.3f at %a differ %llu max_abs %.3e\n", c_wide.u, c_wide.at, (unsigned long long)c_wide.differ, c_wide.abs);
  const bool nan_ok = rgbl::po_sin(1048577.0) != rgbl::po_sin(1048577.0) && rgbl::po_cos(INFINITY) != rgbl::po_cos(INFINITY) &&
                      rgbl::po_sin(NAN) != rgbl::po_sin(NAN);
  printf("beyond the range NaN %d\n", nan_ok ? 1 : 0);
  return nan_ok ? 0 : 1;
}
