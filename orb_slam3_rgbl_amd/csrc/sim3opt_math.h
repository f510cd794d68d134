// sim3opt_math.h — Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) for pinhole key frames, in ONE place for host and
// device: the set-up of an edge pair, the 7-dof vertex, the two binary edges with g2o's numeric Jacobians, Huber, g2o's
// Levenberg and the two rounds, restated from
//   src/Optimizer.cc, include/OptimizableTypes.h:146-215, src/CameraModels/Pinhole.cpp:35-41          (the reference)
//   Thirdparty/g2o/g2o/types/sim3.h:70-146, :233-236, :266-272, core/base_binary_edge.hpp:55-205,
//   core/{optimization_algorithm_levenberg,sparse_optimizer,robust_kernel_impl}.cpp                   (its g2o)
// on top of csrc/poseopt_math.h (sin / cos, Quaterniond(Matrix3d), the quaternion rotation, Huber) and csrc/sim3_math.h
// (the fp32 Rcw * Xw + tcw).  KannalaBrandt8 cameras have no form here.
//
// All arithmetic is fp64 as g2o's is, no contraction (-ffp-contract=off); P3D1c / P3D2c, the normalised obs2 and deltaHuber
// are the reference's floats.  so_exp is fdlibm's __ieee754_exp (e_exp.c), so that host and device give the same bits.
// Against glibc's exp (tests/sim3opt_exp_sweep.cpp, 2^23 arguments over [-1, 1], what sigma of an update can be, and 2^22
// over [-745.2, 709.8]): at most 1 ulp apart on both (9.5 % of the results differ at all); 0, +-inf, NaN, overflow and
// underflow give what libm gives.
//
// The numeric Jacobian IS the function: central differences with delta = 1e-9 (base_binary_edge.hpp:147-197), column d =
// (1 / 2e-9) * (e(+delta e_d) - e(-delta e_d)).  The 14 perturbed estimates Sim3(+-delta e_d) * S and their inverses are the
// same for every edge of a linearisation (the reference recomputes them per edge only because the vertex is shared state);
// they are computed once per linearisation (G.transforms) and an edge pair costs 30 map-and-project evaluations.
//
// What is NOT pinned: the order of Eigen's small fixed-size products - written here left to right -, Eigen's LDLT with its
// pivoting, replaced by lm_solve<7>, libm's exp / sin / cos, and BlockSolverX's dynamic-size products (the 7 x 7 system is
// formed directly).  The solver's failed-pivot rule, the x that persists and g2o's Levenberg with the quirks it keeps are
// stated once, in csrc/lm_math.h.
//
// Quirks of the reference that ARE kept:
//   1. round 1's classification reads the chi2 of the last TRIED step, even a rejected one (:2320; lm_math.h);
//   2. chi2() > th2 compares a double with the float th2 (:2320, :2367);
//   3. nCorrespondences - nBad < 10 returns 0 at :2349: the matches cleared so far stay cleared, g2oS12 is NOT written;
//   4. nMoreIterations is 10 if any pair was dropped, else 5; round 2 starts from the estimate round 1 left, lambda is
//      initialised again at its iteration 0;
//   5. i2 < 0: obs2 is the NORMALISED float (x * invz, y * invz), no intrinsics (:2275-2280).  Its level is the caller's
//      (track_level2).  :2280 names mnTrackScaleLevel but hands it to cv::KeyPoint(Point2f, float size, ...) as the SIZE, so as
//      compiled with OpenCV kpUn2.octave is 0 and :2291 reads mvInvLevelSigma2[0]: the drop-in passes 0, and that is what the
//      reference's own lines give in tests/golden/sim3_opt.  (The member is -1 outside the frustum, Frame.cc:668.)
//   6. the float test P3D2c(2) < 0 lets z == 0 pass: obs2 is then non-finite (i2 < 0), the chi2 NaN, and NaN is never > th2;
//   7. information() * _error is the full 2 x 2 product, zeros included (0 * inf = NaN);
//   8. under _fix_scale oplusImpl zeroes update[6] IN the caller's array: column 6 of every Jacobian is exactly zero, H[6][6]
//      is lambda alone and x[6] = 0;
//   9. a round without edges runs no iteration;
//  10. no quaternion is ever normalised (sim3.h has no normalisation);
//  11. mAcumHessian comes back as zeros (:2356 zeroes it, nothing adds to it): the callers write the zeros.
//  12. tempChi = DBL_MAX after a failed factorisation passes g2o_isfinite (lm_math.h): with an infinite currentChi (a
//      non-finite information) rho is +inf and the step - the x of the last successful solve, or zeros - is ACCEPTED.
//
// Summation order: csrc/lm_math.h's (pair k on lane k mod 256, ascending k, the fixed tree), e12 before e21, for the 28 + 7 + 1
// sums.  Dropped pairs are skipped: a lane's partial sum does not see them.
#pragma once
#include "poseopt_math.h"
#include "sim3_math.h"

namespace rgbl {

constexpr int kSoLanes = kLmLanes;
constexpr int kSoRegEdges = 8;     // edge pairs a lane keeps in registers
constexpr int kSoSums = LmSystem<7>::kSums;   // 36: upper triangle of H (28), b (7), the robust chi2 (1)
constexpr int kSoTransforms = 30;  // S, S^-1, the 14 perturbed estimates, their 14 inverses

// ---- exp ---------------------------------------------------------------------------------------------------------------
RGBL_HD uint64_t so_bits(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
RGBL_HD double so_from_bits(uint64_t u) { double x; __builtin_memcpy(&x, &u, 8); return x; }
// fdlibm's __ieee754_exp
RGBL_HD double so_exp(double x) {
  const double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
               u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
               invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
               P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  const uint64_t bits = so_bits(x);
  const int xsb = (int)(bits >> 63);
  const uint32_t hx = (uint32_t)(bits >> 32) & 0x7fffffffu, lx = (uint32_t)bits;
  double hi = 0.0, lo = 0.0;
  int k = 0;
  if (hx >= 0x40862E42u) {            // |x| >= 709.78
    if (hx >= 0x7ff00000u) {
      if (((hx & 0xfffffu) | lx) != 0) return x + x;   // NaN
      return xsb == 0 ? x : 0.0;      // exp(+-inf)
    }
    if (x > o_threshold) return huge * huge;
    if (x < u_threshold) return twom1000 * twom1000;
  }
  if (hx > 0x3fd62e42u) {             // |x| > 0.5 ln2
    if (hx < 0x3FF0A2B2u) {           // and < 1.5 ln2
      hi = xsb ? x + ln2HI : x - ln2HI;
      lo = xsb ? -ln2LO : ln2LO;
      k = 1 - xsb - xsb;
    } else {
      k = (int)(invln2 * x + (xsb ? -0.5 : 0.5));
      const double t = (double)k;
      hi = x - t * ln2HI;
      lo = t * ln2LO;
    }
    x = hi - lo;
  } else if (hx < 0x3e300000u) {      // |x| < 2^-28
    return 1.0 + x;
  }
  const double t = x * x;
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  if (k >= -1021) return so_from_bits(so_bits(y) + ((uint64_t)(int64_t)k << 52));
  return so_from_bits(so_bits(y) + ((uint64_t)(int64_t)(k + 1000) << 52)) * twom1000;
}

// ---- g2o::Sim3 ---------------------------------------------------------------------------------------------------------
struct SoSim3 { double q[4], t[3], s; };   // r (x y z w), t, s as sim3.h:46-48 holds them
struct SoCam { double fx, fy, cx, cy; };   // Pinhole::mvParameters, floats promoted

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
RGBL_HD void so_map(const SoSim3& S, const double X[3], double P[3]) {
  po_rotate(S.q, X, P);
  P[0] = S.s * P[0] + S.t[0]; P[1] = S.s * P[1] + S.t[1]; P[2] = S.s * P[2] + S.t[2];
}
// Sim3::inverse (:233-236): (r*, r* ((-1 / s) t), 1 / s)
RGBL_HD SoSim3 so_inverse(const SoSim3& S) {
  SoSim3 I;
  I.q[0] = -S.q[0]; I.q[1] = -S.q[1]; I.q[2] = -S.q[2]; I.q[3] = S.q[3];
  const double m = -1.0 / S.s;
  const double v[3] = {m * S.t[0], m * S.t[1], m * S.t[2]};
  po_rotate(I.q, v, I.t);
  I.s = 1.0 / S.s;
  return I;
}
// Sim3(const Vector7d& update) (:70-142): update = (omega, upsilon, sigma)
RGBL_HD SoSim3 so_exp_sim3(const double u[7]) {
  const double sigma = u[6];
  const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double O[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};   // skew(omega)
  SoSim3 E;
  E.s = so_exp(sigma);
  double O2[9], R[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
  const double eps = 0.00001;
  double A, B, C;
  const bool small_angle = theta < eps;
  if (small_angle) {
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
  } else {
    const double a = po_sin(theta) / theta, b = (1.0 - po_cos(theta)) / (theta * theta);
    for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * O[i]) + b * O2[i];
  }
  if (fabs(sigma) < eps) {
    C = 1.0;
    if (small_angle) {
      A = 1.0 / 2.0;
      B = 1.0 / 6.0;
    } else {
      const double theta2 = theta * theta;
      A = (1.0 - po_cos(theta)) / theta2;
      B = (theta - po_sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (E.s - 1.0) / sigma;
    const double sigma2 = sigma * sigma;
    if (small_angle) {
      A = ((sigma - 1.0) * E.s + 1.0) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.0) * E.s) / (sigma2 * sigma);
    } else {
      const double a = E.s * po_sin(theta), b = E.s * po_cos(theta), theta2 = theta * theta, c = theta2 + sigma2;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
    }
  }
  po_quat_from_matrix(R, E.q);
  double W[9];
  for (int i = 0; i < 9; ++i) W[i] = (A * O[i] + B * O2[i]) + C * (i % 4 == 0 ? 1.0 : 0.0);
  for (int r = 0; r < 3; ++r) E.t[r] = (W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5];
  return E;
}
// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:158-167): Sim3(update) * estimate, operator* as sim3.h:266-272
RGBL_HD SoSim3 so_oplus(const double update[7], const SoSim3& S, bool fix_scale) {
  double u[7];
  for (int i = 0; i < 7; ++i) u[i] = update[i];
  if (fix_scale) u[6] = 0.0;
  const SoSim3 E = so_exp_sim3(u);
  SoSim3 N;
  const double* a = E.q; const double* b = S.q;   // Eigen's quaternion product
  N.q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
  N.q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
  N.q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
  N.q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
  double rt[3];
  po_rotate(E.q, S.t, rt);
  for (int r = 0; r < 3; ++r) N.t[r] = E.s * rt[r] + E.t[r];
  N.s = E.s * S.s;
  return N;
}
// the transforms of one linearisation: T[0] = S, T[1] = S^-1, T[2 + 2d] / T[3 + 2d] = Sim3(+delta e_d) * S / Sim3(-delta e_d) * S,
// T[16 + 2d] / T[17 + 2d] their inverses.  so_transform(j) is entry 2 + j (and 16 + j) for j = 0 .. 13.
RGBL_HD SoSim3 so_perturbed(const SoSim3& S, int j, bool fix_scale) {
  double u[7];
  for (int i = 0; i < 7; ++i) u[i] = i == (j >> 1) ? ((j & 1) ? -1e-9 : 1e-9) : 0.0;
  return so_oplus(u, S, fix_scale);
}

// ---- edges ---------------------------------------------------------------------------------------------------------------
// One correspondence: EdgeSim3ProjectXYZ (e12: obs1 against S.map(X2)) and EdgeInverseSim3ProjectXYZ (e21: obs2 against
// S^-1.map(X1)).  The floats are the reference's (cast to double where they are used: exact).
struct SoEdge {
  float X1[3], X2[3], obs1[2], obs2[2], info1, info2;
  uint8_t gone, cleared;   // gone: dropped after round 1 (:2320-2335); cleared: vpMatches1[idx] = NULL (:2323, :2369)
  double chi12, chi21;     // chi2() of the errors computed last
};

// The set-up of one pair (:2189, :2197, :2235, :2245-2292) from the two world positions.  False: P3D2c(2) < 0, no edge.
// oct1 / oct2 index inv_level_sigma2 (the caller has checked or clamped them); i2 < 0 takes the normalised obs2 (quirk 5).
RGBL_HD bool so_make_edge(const float* Rcw1, const float* tcw1, const float* Rcw2, const float* tcw2, const float* Xw1, const float* Xw2,
                          const float* kp1, float info1, bool in_kf2, const float* kp2, float info2, SoEdge& e) {
  s3_transform(Rcw1, tcw1, Xw1, e.X1);
  s3_transform(Rcw2, tcw2, Xw2, e.X2);
  if (e.X2[2] < 0.0f) return false;
  e.obs1[0] = kp1[0]; e.obs1[1] = kp1[1];
  if (in_kf2) {
    e.obs2[0] = kp2[0]; e.obs2[1] = kp2[1];
  } else {
    const float invz = 1.0f / e.X2[2];
    e.obs2[0] = e.X2[0] * invz; e.obs2[1] = e.X2[1] * invz;
  }
  e.info1 = info1; e.info2 = info2;
  e.gone = 0; e.cleared = 0;
  e.chi12 = 0.0; e.chi21 = 0.0;
  return true;
}

// obs - Pinhole::project(T.map(X)) and chi2() = _error.dot(information() * _error) (quirk 7)
RGBL_HD double so_error(const float obs[2], const float X[3], double info, const SoCam& C, const SoSim3& T, double err[2]) {
  const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]};
  double P[3];
  so_map(T, Xd, P);
  err[0] = (double)obs[0] - (C.fx * P[0] / P[2] + C.cx);
  err[1] = (double)obs[1] - (C.fy * P[1] / P[2] + C.cy);
  const double w0 = info * err[0] + 0.0 * err[1], w1 = 0.0 * err[0] + info * err[1];
  return err[0] * w0 + err[1] * w1;
}
// computeError of both edges at estimate S with inverse Si
RGBL_HD void so_edge_errors(SoEdge& e, const SoCam& C1, const SoCam& C2, const SoSim3& S, const SoSim3& Si) {
  double err[2];
  e.chi12 = so_error(e.obs1, e.X2, (double)e.info1, C1, S, err);
  e.chi21 = so_error(e.obs2, e.X1, (double)e.info2, C2, Si, err);
}
RGBL_HD double so_rho(double chi2, bool robust, double delta) {
  if (!robust) return chi2;
  double r0, r1;
  po_huber(chi2, delta, &r0, &r1);
  return r0;
}

// linearizeOplus (base_binary_edge.hpp:131-205) + constructQuadraticForm (:55-120) of one edge: obs against the point X
// through T0 (the error) and Tp[0 .. 13] (the perturbed estimates, + then - per dimension).  Returns the edge's chi2.
RGBL_HD double so_accumulate_one(const float obs[2], const float X[3], double info, const SoCam& C, const SoSim3& T0, const SoSim3* Tp,
                                 bool robust, double delta, double acc[kSoSums]) {
  const double scalar = 1.0 / (2 * 1e-9);
  double err[2], J[2][7] = {};
  const double chi2 = so_error(obs, X, info, C, T0, err);
  // a real loop on the device: unrolled, the 14 evaluations' transforms are all fetched before the first is used
#pragma unroll 1
  for (int d = 0; d < 7; ++d) {
    double ep[2], em[2];
    so_error(obs, X, info, C, Tp[2 * d], ep);
    so_error(obs, X, info, C, Tp[2 * d + 1], em);
    const double j0 = scalar * (ep[0] - em[0]), j1 = scalar * (ep[1] - em[1]);
#pragma unroll
    for (int c = 0; c < 7; ++c) { J[0][c] = c == d ? j0 : J[0][c]; J[1][c] = c == d ? j1 : J[1][c]; }   // J stays in registers
  }
  double rho0 = chi2, rho1 = 1.0;
  if (robust) po_huber(chi2, delta, &rho0, &rho1);
  const double w = rho1 * info;                                             // weightedOmega = rho[1] * information
  const double r0 = -(info * err[0]) * rho1, r1 = -(info * err[1]) * rho1;  // omega_r = -omega * _error; omega_r *= rho[1]
  int k = 0;
  for (int j = 0; j < 7; ++j)
    for (int c = j; c < 7; ++c, ++k) acc[k] = acc[k] + (J[0][j] * (w * J[0][c]) + J[1][j] * (w * J[1][c]));
  for (int j = 0; j < 7; ++j) acc[28 + j] = acc[28 + j] + (J[0][j] * r0 + J[1][j] * r1);
  acc[35] = acc[35] + rho0;
  return chi2;
}
RGBL_HD void so_edge_accumulate(SoEdge& e, const SoCam& C1, const SoCam& C2, const SoSim3* T, bool robust, double delta, double acc[kSoSums]) {
  e.chi12 = so_accumulate_one(e.obs1, e.X2, (double)e.info1, C1, T[0], T + 2, robust, delta, acc);
  e.chi21 = so_accumulate_one(e.obs2, e.X1, (double)e.info2, C2, T[1], T + 16, robust, delta, acc);
}

// what the tests compare besides the estimate, the flags and the count; the first six are rgbl_sim3_opt_diag's counters
struct SoDiag {
  int32_t n_correspondences, n_bad_mps, n_in_kf2, n_out_kf2, n_without_mp, n_bad;
  int32_t iterations[2];   // solve() calls of each optimize() (0: no edge, or not run)
  int32_t active[2];       // edge pairs in the graph when the round began
  double chi2[2];          // the Levenberg currentChi when optimize() returned
  int32_t rounds, reserved;
};

// ---- the optimiser -----------------------------------------------------------------------------------------------------
// `G` owns the problem's edge pairs, the partial sums and the transforms of a linearisation: the lanes of csrc/lm_math.h
// (zero, each, reduce_system, reduce_one) with kSoSums sums, and
//   G.transforms(S, fix_scale)    the kSoTransforms transforms at S, the same for every lane (device: LDS)
// The model lm_levenberg<7> runs: the 7-dof vertex estimate and the two passes over the edge pairs.
struct SoModel {
  const SoCam &C1, &C2;
  SoSim3& S;    // the estimate (the caller's)
  SoSim3 St;    // the one of the trial (written by trial, read by accept)
  bool robust, fix_scale;
  double delta;
  RGBL_HD SoModel(const SoCam& c1, const SoCam& c2, SoSim3& estimate, bool robust_kernel, bool fix, double d)
      : C1(c1), C2(c2), S(estimate), robust(robust_kernel), fix_scale(fix), delta(d) {}
  template <class Lanes> RGBL_HD void linearise(Lanes& G) {
    const SoSim3* T = G.transforms(S, fix_scale);
    G.zero();
    G.each([&](SoEdge& e, double* acc) { if (!e.gone) so_edge_accumulate(e, C1, C2, T, robust, delta, acc); });
  }
  template <class Lanes> RGBL_HD void trial(Lanes& G, double* x) {
    if (fix_scale) x[6] = 0.0;    // quirk 8: oplusImpl writes the zero into the solver's x
    St = so_oplus(x, S, fix_scale);
    const SoSim3 Sti = so_inverse(St);
    G.zero();
    G.each([&](SoEdge& e, double* acc) {
      if (e.gone) return;
      so_edge_errors(e, C1, C2, St, Sti);
      acc[0] = acc[0] + so_rho(e.chi12, robust, delta);
      acc[0] = acc[0] + so_rho(e.chi21, robust, delta);
    });
  }
  RGBL_HD void accept() { S = St; }
};
// SparseOptimizer::optimize(max_it) on the 7-dof vertex: S is the estimate on entry and on return.
template <class Lanes>
RGBL_HD void so_levenberg(Lanes& G, const SoCam& C1, const SoCam& C2, SoSim3& S, bool robust, double delta, bool fix_scale, int max_it,
                          double x[7], int* iterations, double* chi) {
  SoModel M(C1, C2, S, robust, fix_scale, delta);
  lm_levenberg<7>(G, M, max_it, x, iterations, chi);
}

// Optimizer.cc:2306-2380.  D's six counters are the caller's (the set-up); n_corr = nCorrespondences.  Returns nIn, or 0;
// `out` is the entry estimate bit for bit when the function returns at :2349.
template <class Lanes>
RGBL_HD int so_optimize(Lanes& G, const SoCam& C1, const SoCam& C2, const SoSim3& entry, int n_corr, float th2, bool fix_scale,
                        SoSim3& out, SoDiag& D) {
  for (int r = 0; r < 2; ++r) { D.iterations[r] = 0; D.active[r] = 0; D.chi2[r] = 0.0; }
  D.rounds = 0; D.reserved = 0; D.n_bad = 0;
  out = entry;
  const double delta = (double)(float)sqrt((double)th2);   // const float deltaHuber = sqrt(th2) (:2157)
  const double th = (double)th2;
  double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  SoSim3 S = entry;
  int nMore = 5;
  for (int round = 0; round < 2; ++round) {   // one call site: so_levenberg is inlined once
    const int n_active = n_corr - D.n_bad;
    int iters = 0;
    double chi = 0.0;
    if (n_active > 0)                         // :2308 with Huber on every edge, :2353 without
      so_levenberg(G, C1, C2, S, round == 0, delta, fix_scale, round == 0 ? 5 : nMore, x, &iters, &chi);
    if (round == 0) { D.active[0] = n_active; D.iterations[0] = iters; D.chi2[0] = chi; }   // constant indices: D stays in registers
    else { D.active[1] = n_active; D.iterations[1] = iters; D.chi2[1] = chi; }
    D.rounds = round + 1;
    if (round == 1) break;
    G.zero();
    G.each([&](SoEdge& e, double* acc) {      // :2313-2340
      if (e.chi12 > th || e.chi21 > th) { e.gone = 1; e.cleared = 1; acc[0] = acc[0] + 1.0; }
    });
    D.n_bad = (int)G.reduce_one();
    nMore = D.n_bad > 0 ? 10 : 5;
    if (n_corr - D.n_bad < 10) return 0;   // :2348-2349
  }
  const SoSim3 Si = so_inverse(S);
  G.zero();
  G.each([&](SoEdge& e, double* acc) {   // :2357-2374
    if (e.gone) return;
    so_edge_errors(e, C1, C2, S, Si);
    if (e.chi12 > th || e.chi21 > th) e.cleared = 1; else acc[0] = acc[0] + 1.0;
  });
  const int nIn = (int)G.reduce_one();
  out = S;
  return nIn;
}

// The host's execution of the lanes: csrc/lm_math.h's, and the transforms.
struct SoHostLanes : LmHostLanes<SoEdge, kSoSums> {
  SoSim3 T[kSoTransforms];
  using LmHostLanes::LmHostLanes;
  const SoSim3* transforms(const SoSim3& S, bool fix_scale) {
    T[0] = S;
    T[1] = so_inverse(S);
    for (int j = 0; j < 14; ++j) { T[2 + j] = so_perturbed(S, j, fix_scale); T[16 + j] = so_inverse(T[2 + j]); }
    return T;
  }
};

}  // namespace rgbl
