// The host build of csrc/twoview_math.h as a stand-alone program: tests/test_twoview_math.py compiles it with
// -fsanitize=address,undefined and runs it.  It is never loaded into Python.
//   1. tv_acosf against libm's acosf over a sweep of [-1, 1] and the cosines CheckRT sees (1 - 2^-k): both are within an ulp
//      of the exact value, so they may differ by 2 ulp at the most.
//   2. the null vector of the 16 x 9 and 8 x 9 matrices against a residual bound: |A v| <= sigma_min + 1e-6 * sigma_max, with
//      sigma_min, sigma_max from a cyclic Jacobi on A^T A of 60 sweeps written here (v is rounded to float: 9 components of
//      relative error 2^-24 move A v by less than 2e-7 * sigma_max; the rest is the margin for the 12 sweeps of the header).
//   3. every function of the header on a general scene, a planar scene, coincident and collinear sets and a frame whose keys
//      share one x (sX = inf): no out-of-bounds access, no undefined conversion on any of these paths, and the planted motion
//      is among the hypotheses where the scene has one.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "twoview_math.h"

using namespace rgbl;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static double uniform(double lo, double hi) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return lo + (hi - lo) * (double)(rng_state >> 11) / 9007199254740992.0;
}
static int ulps(float a, float b) {
  int32_t x, y;
  memcpy(&x, &a, 4); memcpy(&y, &b, 4);
  return abs(x - y);
}

static void check_acos() {
  int worst = 0;
  float at = 0.0f;
  for (int i = 0; i <= 2000000; ++i) {
    const float x = (float)(-1.0 + (double)i * 1e-6);
    const int d = ulps(tv_acosf(x), acosf(x));
    if (d > worst) { worst = d; at = x; }
  }
  for (int k = 1; k < 25; ++k) {
    const float x = 1.0f - ldexpf(1.0f, -k);
    const int d = ulps(tv_acosf(x), acosf(x));
    if (d > worst) { worst = d; at = x; }
  }
  printf("acos: at most %d ulp from libm's acosf (at %.9g)\n", worst, at);
  CHECK(worst <= 2);
  CHECK(tv_acosf(1.0f) == 0.0f);
  CHECK(tv_acosf(1.5f) != tv_acosf(1.5f));   // NaN, as libm's
  CHECK(fabsf(tv_parallax_deg(0.0f) - 90.0f) < 1e-5f);
}

// two frames of n keys, every key matched with its namesake
struct Scene {
  std::vector<float> xy1, xy2;
  std::vector<int32_t> m1, m2;
  TvView v;
  double R[9], t[3];
  Scene(int n, bool planar, bool rotation_only) : xy1(2 * n), xy2(2 * n), m1(n), m2(n) {
    const float K[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
    const double w[3] = {0.01, 0.05, -0.02};
    ml_rodrigues2rot(w, R);
    t[0] = rotation_only ? 0.0 : -1.2; t[1] = rotation_only ? 0.0 : 0.1; t[2] = rotation_only ? 0.0 : 0.15;
    for (int i = 0; i < n; ++i) {
      const double u = uniform(40, 1200), w2 = uniform(40, 330);
      const double x = (u - K[2]) / K[0], y = (w2 - K[3]) / K[1];
      const double z = planar ? 9.0 / (0.25 * x - 0.1 * y + 1.0) : uniform(4, 40);
      const double X[3] = {x * z, y * z, z};
      double Y[3];
      ml_matvec(R, X, Y);
      for (int c = 0; c < 3; ++c) Y[c] += t[c];
      xy1[2 * i] = (float)u; xy1[2 * i + 1] = (float)w2;
      xy2[2 * i] = (float)(K[0] * Y[0] / Y[2] + K[2]); xy2[2 * i + 1] = (float)(K[1] * Y[1] / Y[2] + K[3]);
      m1[i] = i; m2[i] = i;
    }
    v.xy1 = xy1.data(); v.xy2 = xy2.data(); v.m1 = m1.data(); v.m2 = m2.data(); v.N = n; v.n1 = n; v.n2 = n; v.sigma = 1.0f;
    memcpy(v.K, K, sizeof(K));
    normalize();
  }
  void normalize() {
    TvHostX x;
    float buf[2][64];
    tv_normalize(x, buf, v.xy1, v.n1, v.T1);
    tv_normalize(x, buf, v.xy2, v.n2, v.T2);
  }
};

static std::vector<TvWork> work(1);

// sigma_min and sigma_max of the set's A by 60 sweeps, and |A v| of the header's vector
static void residual(const Scene& s, const int32_t* set, bool fundamental, double* smin, double* smax, double* res) {
  const int nrows = fundamental ? 8 : 16;
  double A[16][9], B[9][9];
  for (int r = 0; r < nrows; ++r) tv_row(s.v, set, fundamental, r, A[r]);
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) { B[i][j] = 0.0; for (int r = 0; r < nrows; ++r) B[i][j] += A[r][i] * A[r][j]; }
  for (int sweep = 0; sweep < 60; ++sweep)
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        double c, sn, tt;
        ml_jacobi_cs(B[p][p], B[q][q], B[p][q], &c, &sn, &tt);
        for (int r = 0; r < 9; ++r) { const double a = B[r][p], b = B[r][q]; B[r][p] = c * a - sn * b; B[r][q] = sn * a + c * b; }
        for (int r = 0; r < 9; ++r) { const double a = B[p][r], b = B[q][r]; B[p][r] = c * a - sn * b; B[q][r] = sn * a + c * b; }
      }
  double lo = B[0][0], hi = B[0][0];
  for (int i = 1; i < 9; ++i) { lo = B[i][i] < lo ? B[i][i] : lo; hi = B[i][i] > hi ? B[i][i] : hi; }
  *smin = sqrt(lo > 0.0 ? lo : 0.0);
  *smax = sqrt(hi);
  TvHostX x;
  float h[9];
  tv_null_vector(x, work[0], s.v, set, fundamental, h);
  double n2 = 0.0, top = 0.0;
  int arg = 0;
  for (int i = 0; i < 9; ++i) { n2 += (double)h[i] * h[i]; if (fabs((double)h[i]) > top) { top = fabs((double)h[i]); arg = i; } }
  CHECK(fabs(sqrt(n2) - 1.0) < 1e-6);
  CHECK(h[arg] > 0.0f);   // the sign rule
  double r2 = 0.0;
  for (int r = 0; r < nrows; ++r) { double d = 0.0; for (int c = 0; c < 9; ++c) d += A[r][c] * (double)h[c]; r2 += d * d; }
  *res = sqrt(r2);
}

static void check_null_vectors() {
  double worst = 0.0;
  for (int scene = 0; scene < 3; ++scene) {
    Scene s(120, scene == 1, scene == 2);
    for (int k = 0; k < 200; ++k) {
      int32_t set[8];
      for (int j = 0; j < 8; ++j) {
        bool again = true;
        while (again) {
          set[j] = (int32_t)uniform(0, 119.999);
          again = false;
          for (int i = 0; i < j; ++i) again = again || set[i] == set[j];
        }
      }
      for (int fundamental = 0; fundamental < 2; ++fundamental) {
        double smin, smax, res;
        residual(s, set, fundamental != 0, &smin, &smax, &res);
        const double over = (res - smin) / smax;
        worst = over > worst ? over : worst;
        CHECK(res <= smin + 1e-6 * smax);
      }
    }
  }
  printf("null vector: |A v| exceeds sigma_min by at most %.3g of sigma_max\n", worst);
}

// the whole chain on one scene with one set; returns the inliers of the model
static int chain(Scene& s, const int32_t* set, int model, bool expect_motion) {
  TvHostX x;
  float M[9], M2[9];
  tv_model(x, work[0], s.v, set, model, M, M2);
  const float inv = tv_inv_sigma2(s.v.sigma);
  float score = 0.0f;
  std::vector<uint8_t> in((size_t)s.v.N);
  int count = 0;
  for (int i = 0; i < s.v.N; ++i) {
    float t[2];
    in[(size_t)i] = tv_check(model, M, M2, s.v, i, inv, t) ? 1 : 0;
    count += in[(size_t)i];
    score = tv_add_chunk(score, t, 2);
  }
  TvMotions mo;
  mo.n = 0;
  if (model == 0) tv_motions_h(M, s.v.K, mo); else tv_motions_f(M, s.v.K, mo);
  int32_t nGood[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float par[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double closest = 1e9;
  const double tn = sqrt(s.t[0] * s.t[0] + s.t[1] * s.t[1] + s.t[2] * s.t[2]);
  for (int j = 0; j < mo.n; ++j) {
    TvCam c;
    tv_cam(s.v.K, mo.R[j], mo.t[j], s.v.sigma, c);
    for (int i = 0; i < s.v.N; ++i) {
      if (!in[(size_t)i]) continue;
      float p[3], cp;
      nGood[j] += tv_rt_point(c, s.xy1[2 * i], s.xy1[2 * i + 1], s.xy2[2 * i], s.xy2[2 * i + 1], p, &cp) ? 1 : 0;
    }
    par[j] = tv_parallax_deg(0.9995f);
    double d = 0.0;
    for (int k = 0; k < 9; ++k) d = fmax(d, fabs((double)mo.R[j][k] - s.R[k]));
    for (int k = 0; k < 3 && tn > 0.0; ++k) d = fmax(d, fabs((double)mo.t[j][k] - s.t[k] / tn));
    closest = d < closest ? d : closest;
  }
  const TvDecision d = model == 0 ? tv_decide_h(nGood, par, count) : tv_decide_f(nGood, par, count);
  (void)d;
  if (expect_motion) { CHECK(score > 0.0f); CHECK(count > s.v.N / 2); CHECK(closest < 1e-2); }
  return count;
}

static void check_chain() {
  const int32_t set[8] = {3, 17, 29, 41, 58, 73, 90, 111}, same[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  Scene g(120, false, false), p(120, true, false), r(120, false, true);
  chain(g, set, 1, true);
  chain(g, set, 0, false);
  chain(p, set, 0, true);
  chain(p, set, 1, false);
  chain(r, set, 0, false);      // d1 == d2 == d3: no motion hypotheses
  chain(r, set, 1, false);
  Scene c(120, false, false);
  for (int j = 1; j < 8; ++j) { c.xy1[2 * j] = c.xy1[0]; c.xy1[2 * j + 1] = c.xy1[1]; c.xy2[2 * j] = c.xy2[0]; c.xy2[2 * j + 1] = c.xy2[1]; }
  c.normalize();
  chain(c, same, 0, false);     // coincident
  chain(c, same, 1, false);
  Scene l(120, false, false);
  for (int j = 0; j < 8; ++j) { l.xy1[2 * j] = 100.0f + 30.0f * j; l.xy1[2 * j + 1] = 50.0f + 15.0f * j; l.xy2[2 * j] = 120.0f + 32.0f * j; l.xy2[2 * j + 1] = 60.0f + 16.0f * j; }
  l.normalize();
  chain(l, same, 0, false);     // collinear
  chain(l, same, 1, false);
  Scene f(120, false, false);
  for (int i = 0; i < 120; ++i) f.xy2[2 * i] = 321.5f;
  f.normalize();
  CHECK(f.v.T2[0] > FLT_MAX);   // sX = 1.0 / 0
  CHECK(chain(f, set, 0, false) >= 0);
  chain(f, set, 1, false);
  CHECK(tv_choose_model(0.0f, 0.0f) == -1 && tv_choose_model(1.0f, 0.0f) == 0 && tv_choose_model(0.0f, 1.0f) == 1 && tv_choose_model(1.0f, 1.0f) == 1);
  const float sc[8] = {1.0f, 0.0f, NAN, 2.0f, 3.0f, NAN, 3.0f, 5.0f};
  float best;
  CHECK(tv_first_max(sc, 4, 0, &best) == 2 && best == 3.0f);   // the first of the equal maxima; the NaN before it does not win
  CHECK(tv_first_max(sc, 4, 1, &best) == 3 && best == 5.0f);
  const float none[4] = {0.0f, NAN, -1.0f, NAN};
  CHECK(tv_first_max(none, 2, 0, &best) == -1 && best == 0.0f);
}

int main() {
  check_acos();
  check_null_vectors();
  check_chain();
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("TWOVIEW_HOST_CHECK_OK\n");
  return 0;
}
