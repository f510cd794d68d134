// The host build of csrc/mlpnp_math.h on seeded, planar and degenerate sets, as a stand-alone program: tests/test_mlpnp_math.py
// compiles it with -fsanitize=address,undefined and runs it (no out-of-bounds access, no undefined conversion or shift on any of
// these paths).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mlpnp_math.h"

using namespace rgbl;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static double uniform(double lo, double hi) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return lo + (hi - lo) * (double)(rng_state >> 11) / 9007199254740992.0;
}

// a scene of n correspondences under the pose (w, t): every feature carries a map point, exact observations
struct Scene {
  std::vector<float> xy, wpos, sigma2;
  std::vector<int32_t> oct, feat, point, list;
  MlView v;
  Scene(int n, const double* w, const double* t, bool planar) : xy(2 * n), wpos(3 * n), sigma2(8), oct(n), feat(n), point(n), list(n) {
    double R[9];
    ml_rodrigues2rot(w, R);
    const float K[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};
    for (int l = 0; l < 8; ++l) sigma2[l] = (float)pow(1.2, 2 * l);
    for (int i = 0; i < n; ++i) {
      double X[3];
      if (planar) { X[0] = floor(uniform(-6, 6) * 64) / 64; X[1] = floor(uniform(-2.5, 2.5) * 64) / 64; X[2] = 0.0; }
      else { X[0] = uniform(-8, 8); X[1] = uniform(-4, 4); X[2] = uniform(-6, 6); }
      for (int c = 0; c < 3; ++c) wpos[3 * i + c] = (float)X[c];
      const double Xf[3] = {wpos[3 * i], wpos[3 * i + 1], wpos[3 * i + 2]};
      double Y[3];
      ml_matvec(R, Xf, Y);
      for (int c = 0; c < 3; ++c) Y[c] += t[c];
      xy[2 * i] = (float)(K[0] * Y[0] / Y[2] + K[2]);
      xy[2 * i + 1] = (float)(K[1] * Y[1] / Y[2] + K[3]);
      oct[i] = i % 8; feat[i] = i; point[i] = i; list[i] = i;
    }
    v.xy = xy.data(); v.oct = oct.data(); v.wpos = wpos.data(); v.sigma2 = sigma2.data(); v.feat = feat.data(); v.point = point.data();
    v.N = n; v.n_levels = 8; v.th2 = 5.991f;
    memcpy(v.K, K, sizeof(K));
  }
  int count(const double* R, const double* t) const {
    int c = 0;
    for (int i = 0; i < v.N; ++i) c += ml_is_inlier(v, R, t, i) ? 1 : 0;
    return c;
  }
};

static std::vector<MlWork> work(1);

static int pose_six(const Scene& s, const int32_t* sample, double* R, double* t) {
  MlHostX x;
  MlSixSums Q;
  const MlSet S = {&s.v, sample, 6};
  int path;
  ml_compute_pose(x, work[0], Q, S, R, t, &path);
  return path;
}
static bool finite9(const double* R) {
  for (int i = 0; i < 9; ++i)
    if (!ml_finite(R[i])) return false;
  return true;
}

int main() {
  const double w[3] = {0.1, -0.2, 0.15}, t[3] = {0.3, -0.2, 14.0};
  double Rt[9];
  ml_rodrigues2rot(w, Rt);
  // 1. exact observations: a six-point set recovers the pose
  {
    Scene s(700, w, t, false);
    const int32_t sample[6] = {3, 77, 201, 5, 640, 333};
    double R[9], tt[3];
    const int path = pose_six(s, sample, R, tt);
    CHECK((path & 16) != 0);
    for (int i = 0; i < 9; ++i) CHECK(fabs(R[i] - Rt[i]) < 1e-5);
    for (int i = 0; i < 3; ++i) CHECK(fabs(tt[i] - t[i]) < 1e-3);
    CHECK(s.count(R, tt) == 700);
  }
  // 2. a planar scene: rank 2, the 9-column branch runs to the end with finite results
  {
    Scene s(300, w, t, true);
    double M[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 300; ++i) {
      const double X[3] = {s.wpos[3 * i], s.wpos[3 * i + 1], s.wpos[3 * i + 2]};
      M[0] += X[0] * X[0]; M[1] += X[0] * X[1]; M[2] += X[0] * X[2]; M[3] += X[1] * X[1]; M[4] += X[1] * X[2]; M[5] += X[2] * X[2];
    }
    CHECK(ml_rank3(M) == 2);
    double E[9];
    ml_eigen_frame(M, E);
    CHECK(fabs(fabs(E[2]) - 1.0) < 1e-12);   // the normal first
    double R[9], tt[3];
    const int32_t sample[6] = {0, 50, 100, 150, 200, 250};
    pose_six(s, sample, R, tt);
    CHECK(finite9(R));
  }
  // 3. the rank rule
  {
    const double full[6] = {2, 0, 0, 3, 0, 4}, two[6] = {2, 0, 0, 3, 0, 0}, one[6] = {1, 2, 3, 4, 6, 9}, zero[6] = {0, 0, 0, 0, 0, 0};
    const double nan[6] = {NAN, 0, 0, 1, 0, 1}, tiny[6] = {1, 0, 0, 1, 0, 1e-17}, small[6] = {1, 0, 0, 1, 0, 1e-15};
    CHECK(ml_rank3(full) == 3 && ml_rank3(two) == 2 && ml_rank3(one) == 1 && ml_rank3(zero) == 0 && ml_rank3(nan) == 0);
    CHECK(ml_rank3(tiny) == 2 && ml_rank3(small) == 3);   // the threshold is 3 * 2.2e-16 of the largest pivot
  }
  // 4. degenerate sets run to the end: coincident points, points on a line through the origin, non-finite coordinates
  {
    Scene s(40, w, t, false);
    for (int i = 1; i < 6; ++i) for (int c = 0; c < 3; ++c) s.wpos[3 * i + c] = s.wpos[c];
    for (int i = 6; i < 12; ++i) { s.wpos[3 * i] = 0.5f * (i - 4); s.wpos[3 * i + 1] = 0.25f * (i - 4); s.wpos[3 * i + 2] = 1.0f * (i - 4); }
    s.wpos[3 * 12] = NAN; s.wpos[3 * 13 + 1] = INFINITY;
    double R[9], tt[3];
    const int32_t a[6] = {0, 1, 2, 3, 4, 5}, b[6] = {6, 7, 8, 9, 10, 11}, c[6] = {12, 13, 14, 15, 16, 17};
    pose_six(s, a, R, tt);
    CHECK(s.count(R, tt) >= 0);
    pose_six(s, b, R, tt);
    CHECK(s.count(R, tt) >= 0);
    const int path = pose_six(s, c, R, tt);
    CHECK(!finite9(R) || path >= 0);
    CHECK(s.count(R, tt) <= 40);
  }
  // 5. a pose of exactly identity: rot2rodrigues gives w = 0 for a trace of 3 or more, the Jacobian there is NaN, x stays
  {
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double om[3];
    ml_rot2rodrigues(I9, om);
    CHECK(om[0] == 0.0 && om[1] == 0.0 && om[2] == 0.0);
    const double past[9] = {1 + 1e-15, 0, 0, 0, 1, 0, 0, 0, 1};
    ml_rot2rodrigues(past, om);
    CHECK(om[0] == 0.0 && om[1] == 0.0 && om[2] == 0.0);   // acos of an argument past 1: NaN fails the guard
    const double x0[6] = {0, 0, 0, 0.1, 0.2, 5.0};
    MlGn G;
    ml_gn_state(x0, G);
    const double f[3] = {0.1, -0.2, 1.0}, X[3] = {1, 2, 3};
    double res[2], J0[6], J1[6];
    ml_gn_rows(G, f, X, res, J0, J1);
    CHECK(J0[0] != J0[0] && ml_finite(J0[3]) && ml_finite(res[0]));
    const double z[3] = {0, 0, 0};
    Scene s(30, z, z, false);
    for (int i = 0; i < 30; ++i) s.wpos[3 * i + 2] += 12.0f;   // in front of the camera; observations are recomputed below
    for (int i = 0; i < 30; ++i) {
      s.xy[2 * i] = s.v.K[0] * s.wpos[3 * i] / s.wpos[3 * i + 2] + s.v.K[2];
      s.xy[2 * i + 1] = s.v.K[1] * s.wpos[3 * i + 1] / s.wpos[3 * i + 2] + s.v.K[3];
    }
    double R[9], tt[3];
    const int32_t six[6] = {0, 5, 10, 15, 20, 25};
    pose_six(s, six, R, tt);
    CHECK(s.count(R, tt) == 30);
  }
  // 6. the header's own functions
  {
    CHECK(fabs(ml_cbrt(27.0) - 3.0) < 1e-15 && fabs(ml_cbrt(1e-30) - 1e-10) < 1e-25 && fabs(ml_cbrt(8e300) / 2e100 - 1.0) < 1e-15);
    CHECK(ml_cbrt(0.0) == 0.0 && ml_cbrt(NAN) != ml_cbrt(NAN) && ml_cbrt(INFINITY) == INFINITY);
    double worst = 0.0;
    for (int i = 0; i < 200000; ++i) {
      const double x = uniform(1e-3, 1e3), y = ml_cbrt(x);
      worst = fmax(worst, fabs(y - cbrt(x)) / cbrt(x));
    }
    CHECK(worst < 1e-15);   // a few ulp: the last Newton step rounds four times
    worst = 0.0;
    for (int i = 0; i < 200000; ++i) {
      const double x = uniform(-1.0, 1.0);
      worst = fmax(worst, fabs(ml_acos(x) - acos(x)));
    }
    CHECK(worst < 1e-8 && ml_acos(1.0) == 0.0 && ml_acos(1.0000001) != ml_acos(1.0000001));
    printf("cbrt and acos against libm: ok\n");
    CHECK(ml_sum6(1, 2, 3, 4, 5, 6) == 21.0);
    for (int step = 0; step < 11; ++step) {   // every step of the round-robin pairs every index once
      int seen = 0;
      for (int k = 0; k < 6; ++k) { int p, q; ml_pair(k, step, 11, &p, &q); CHECK(p < q && q < 12); seen |= (1 << p) | (1 << q); }
      CHECK(seen == 0xfff);
    }
  }
  // 7. the scan's corners: Refine as compiled succeeds iff c[k] > min_inliers and returns hypothesis k
  {
    const int32_t c[6] = {3, 10, 12, 9, 12, 20};
    MlScan r = ml_scan(c, 6, 10, 0);
    CHECK(r.found == 1 && r.no_more == 0 && r.iterations == 3 && r.selected == 2 && r.record == 2 && r.refines == 2 && r.n_inliers == 12 && r.best == 12);
    r = ml_scan(c, 6, 12, 0);   // 12 == min qualifies, twice, without success; the first is the record; 20 succeeds
    CHECK(r.found == 1 && r.iterations == 6 && r.selected == 5 && r.record == 5 && r.refines == 3 && r.n_inliers == 20);
    r = ml_scan(c, 5, 12, 0);   // runs through: the first 12 is the record
    CHECK(r.found == 1 && r.no_more == 1 && r.selected == -1 && r.record == 2 && r.refines == 2 && r.n_inliers == 12 && r.iterations == 5);
    r = ml_scan(c, 6, 10, 15);  // a larger record carried in: the success at 12 is not the record
    CHECK(r.found == 1 && r.selected == 2 && r.record == -1 && r.best == 15 && r.n_inliers == 12 && r.refines == 2);
    r = ml_scan(c, 6, 21, 0);
    CHECK(r.found == 0 && r.no_more == 1 && r.refines == 0 && r.iterations == 6 && r.selected == -1);
    r = ml_scan(c, 6, 21, 25);  // nothing qualifies: the carried record is handed out
    CHECK(r.found == 1 && r.no_more == 1 && r.n_inliers == 25 && r.record == -1);
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("MLPNP_HOST_CHECK_OK\n");
  return 0;
}
