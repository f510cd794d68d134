// The host build of csrc/sim3_math.h on its degenerate and edge cases, as a stand-alone program: tests/test_sim3_math.py
// compiles it with -fsanitize=address,undefined and runs it (no out-of-bounds access, no undefined conversion or shift on any of
// these paths), and reads the atan2 sweep it prints.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sim3_math.h"

using namespace rgbl;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool all_nan(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (v[i] == v[i]) return false;
  return true;
}
static bool all_finite(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(v[i])) return false;
  return true;
}

static double ulps(double a, double b) {
  if (a == b) return 0.0;
  const double u = fabs(nextafter(b, INFINITY) - b);
  return fabs(a - b) / u;
}

int main() {
  const float K[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
  // 1. a rotation about z by 90 degrees, scale 2, translation (1, 2, 3): X1 = 2 R X2 + t
  {
    const float P2[9] = {1, 0, 5, 0, 1, 6, 1, 1, 9};
    float P1[9];
    for (int k = 0; k < 3; ++k) {
      P1[3 * k] = 2 * -P2[3 * k + 1] + 1; P1[3 * k + 1] = 2 * P2[3 * k] + 2; P1[3 * k + 2] = 2 * P2[3 * k + 2] + 3;
    }
    S3Hyp H;
    s3_compute_sim3(P1, P2, 0, H);
    CHECK(fabsf(H.s - 2.0f) < 1e-5f && fabsf(H.R[1] + 1.0f) < 1e-6f && fabsf(H.R[3] - 1.0f) < 1e-6f && fabsf(H.R[8] - 1.0f) < 1e-6f);
    CHECK(fabsf(H.t[0] - 1.0f) < 1e-4f && fabsf(H.t[1] - 2.0f) < 1e-4f && fabsf(H.t[2] - 3.0f) < 1e-4f);
    s3_compute_sim3(P1, P2, 1, H);
    CHECK(H.s == 1.0f);
    // the inverse maps back
    float y[3], x[3] = {P1[0], P1[1], P1[2]};
    s3_compute_sim3(P1, P2, 0, H);
    s3_transform(H.iR, H.it, x, y);
    CHECK(fabsf(y[0] - P2[0]) < 1e-4f && fabsf(y[1] - P2[1]) < 1e-4f && fabsf(y[2] - P2[2]) < 1e-4f);
  }
  // 2. identical sets: the identity, through SO3f::exp's small-angle branch
  {
    const float P[9] = {1, 0, 5, 0, 1, 6, 1, 1, 9};
    S3Hyp H;
    s3_compute_sim3(P, P, 0, H);
    CHECK(all_finite(H.R, 9) || all_nan(H.R, 9));   // w = 1 exactly gives vec.norm() == 0: NaN, as in the reference
  }
  // 3. coincident points: NaN everywhere, no inlier
  {
    const float P[9] = {1, 2, 5, 1, 2, 5, 1, 2, 5};
    S3Hyp H;
    s3_compute_sim3(P, P, 0, H);
    float T[16];
    s3_T12(H, T);
    CHECK(all_nan(T, 12) && T[15] == 1.0f && all_nan(H.iR, 9) && all_nan(H.it, 3));
    const float x[3] = {1, 2, 5};
    const S3Point p = s3_point(x, x, K, K, 1e30f, 1e30f);
    CHECK(!s3_is_inlier(H, K, K, p));
    s3_compute_sim3(P, P, 1, H);
    CHECK(all_nan(H.R, 9) && H.s == 1.0f);
  }
  // 4. collinear points, and collinear in one set only
  {
    const float A[9] = {0, 0, 4, 1, 0.5f, 5, 2, 1, 6};
    const float B[9] = {0, 0, 4, 1, 0, 5, 0, 1, 6};
    S3Hyp H;
    s3_compute_sim3(A, A, 0, H);
    s3_compute_sim3(A, B, 0, H);
    s3_compute_sim3(B, A, 1, H);
    CHECK(H.s == 1.0f);
  }
  // 5. non-finite and huge coordinates
  {
    const float big = 3e38f, inf = INFINITY, nan = NAN;
    const float vals[5] = {big, inf, nan, -big, 1e-45f};
    for (int v = 0; v < 5; ++v) {
      float A[9] = {0, 0, 4, 1, 0.5f, 5, 2, -1, 6}, B[9] = {0, 1, 4, 1, 0, 5, 0, 1, 7};
      A[4] = vals[v];
      S3Hyp H;
      s3_compute_sim3(A, B, 0, H);
      B[8] = vals[v];
      s3_compute_sim3(A, B, 1, H);
      const S3Point p = s3_point(A + 3, B + 6, K, K, 10.0f, 10.0f);
      (void)s3_is_inlier(H, K, K, p);
    }
  }
  // 6. z == 0 and 0 / 0 in the projections
  {
    const float P2[9] = {1, 0, 5, 0, 1, 6, 1, 1, 9};
    float P1[9];
    for (int k = 0; k < 9; ++k) P1[k] = P2[k] + 0.5f;
    S3Hyp H;
    s3_compute_sim3(P1, P2, 0, H);
    const float a[3] = {1, 1, 0}, z[3] = {0, 0, 0}, g[3] = {1.5f, 0.5f, 5.5f}, g2[3] = {1, 0, 5};
    float uv[2];
    s3_pinhole(K, a, uv);
    CHECK(isinf(uv[0]) && isinf(uv[1]));
    s3_pinhole(K, z, uv);
    CHECK(uv[0] != uv[0]);
    CHECK(!s3_is_inlier(H, K, K, s3_point(a, g2, K, K, 1e30f, 1e30f)));
    CHECK(!s3_is_inlier(H, K, K, s3_point(g, z, K, K, 1e30f, 1e30f)));
    CHECK(s3_is_inlier(H, K, K, s3_point(g, g2, K, K, 1.0f, 1.0f)));
  }
  // 7. the selection scan: empty, ties, a stop, a carried-in best
  {
    S3Selection r = s3_select(nullptr, 0, 0, 5);
    CHECK(r.selected == -1 && r.converged == 0 && r.iterations == 0);
    const int32_t c[6] = {2, 4, 4, 9, 12, 3};
    r = s3_select(c, 6, 0, 100);
    CHECK(r.selected == 4 && !r.converged && r.iterations == 6 && r.n_inliers == 12);
    r = s3_select(c, 3, 0, 100);
    CHECK(r.selected == 2 && r.n_inliers == 4);
    r = s3_select(c, 6, 0, 8);
    CHECK(r.selected == 3 && r.converged && r.iterations == 4 && r.n_inliers == 9);
    r = s3_select(c, 6, 13, 8);
    CHECK(r.selected == -1 && !r.converged && r.iterations == 6 && r.n_inliers == 0);
    r = s3_select(c, 6, 12, 20);
    CHECK(r.selected == 4);
  }
  // 8. atan2: the special values, and a sweep against libm
  {
    CHECK(s3_atan2(0.0, 1.0) == 0.0 && s3_atan2(0.0, 0.0) == 0.0 && s3_atan2(1.0, 0.0) == M_PI_2 && s3_atan2(1.0, 1.0) == M_PI_4);
    CHECK(s3_atan2(NAN, 1.0) != s3_atan2(NAN, 1.0) && s3_atan2(1.0, NAN) != s3_atan2(1.0, NAN));
    CHECK(s3_atan2(INFINITY, INFINITY) == M_PI_4 && s3_atan2(INFINITY, 1.0) == M_PI_2 && s3_atan2(1.0, INFINITY) == 0.0);
    CHECK(s3_atan2(0.0, -1.0) == M_PI && s3_atan2(-1.0, 0.0) == -M_PI_2);
    double worst1 = 0.0, worst = 0.0;
    unsigned s = 12345u;
    for (int i = 0; i < 2000000; ++i) {
      s = s * 1664525u + 1013904223u;
      const double a = (double)(s >> 8) / 16777216.0;
      s = s * 1664525u + 1013904223u;
      const double b = (double)(s >> 8) / 16777216.0;
      // unit vectors rounded to float, as the solver's arguments are
      const double nrm = sqrt(a * a + b * b);
      if (nrm == 0.0) continue;
      const double y = (double)(float)(a / nrm), x = (double)(float)(b / nrm);
      const double u = ulps(s3_atan2(y, x), atan2(y, x));
      if (u > worst1) worst1 = u;
      const double sy = (i & 1) ? -y : y, sx = (i & 2) ? -x : x;
      const double u2 = ulps(s3_atan2(sy * 1e-3, sx * 37.0), atan2(sy * 1e-3, sx * 37.0));
      const double u3 = ulps(s3_atan2(sy, sx), atan2(sy, sx));
      if (u2 > worst) worst = u2;
      if (u3 > worst) worst = u3;
    }
    printf("atan2 first_quadrant max_ulp %.3f all_quadrants max_ulp %.3f\n", worst1, worst);
  }
  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("SIM3_HOST_CHECK_OK\n");
  return 0;
}
