// poseopt_math.h — Optimizer::PoseOptimization (src/Optimizer.cc:814-1114) for single-camera pinhole frames, in ONE place for
// host and device: set-up, the two edge types, Huber, g2o's Levenberg, the SE3 update and the four rounds, restated from
//   src/Optimizer.cc, src/OptimizableTypes.cpp, src/CameraModels/Pinhole.cpp            (the reference)
//   Thirdparty/g2o/g2o/core/{optimization_algorithm_levenberg,sparse_optimizer,robust_kernel_impl}.cpp,
//   core/{base_edge.h,base_unary_edge.hpp,block_solver.hpp}, solvers/linear_solver_dense.h,
//   types/{se3quat.h,se3_ops.hpp,types_six_dof_expmap.{h,cpp}}                           (its g2o)
// The rig branch (:930-991), KannalaBrandt8 and the inertial variants have no form here.
//
// All arithmetic is fp64 as g2o's is, no contraction (-ffp-contract=off); division and square root are IEEE on host and device.
// po_sin / po_cos are the header's own (fdlibm's kernels behind a two-term Cody-Waite reduction), so that host and device give
// the same bits; pow(theta, 3) is written as two multiplications.  Supported argument range |x| <= 2^20 (NaN beyond, and for a
// non-finite argument).  Against glibc's sin / cos (tests/poseopt_sincos_sweep.cpp, 2^23 + 2^22 arguments): on [-8, 8], what
// theta = |omega| of an update can be, at most 1 ulp apart (6 % of the results differ at all); over [1e-9, 2^20] the absolute
// difference stays at 1.1e-16, which next to a zero of the function is up to 11 ulp of the result.
//
// What is NOT pinned (as for every Eigen evaluation order in this project): the order of Eigen's small fixed-size products -
// written here left to right -, Eigen's LDLT with its pivoting, replaced by lm_solve<6>, and libm's sin / cos.  The solver's
// failed-pivot rule, the x that persists and g2o's Levenberg with the quirks it keeps are stated once, in csrc/lm_math.h.
//
// Quirks of the reference that ARE kept:
//   1. every round restarts from the ENTRY pose (:1008-1009 read pFrame->GetPose(), not written before :1111);
//   2. after a round an active edge keeps the chi2 of the last TRIED step, even a rejected one; only outlier edges are
//      re-evaluated at the round's final estimate (:1021-1024, :1079-1082);
//   3. `const float chi2 = e->chi2()` is compared with the float thresholds 5.991f / 7.815f;
//   4. the robust kernel is dropped after round index 2;
//   5. `optimizer.edges().size() < 10` is decided by nInitialCorrespondences alone;
//   6. fewer than 3 correspondences: return 0, pose untouched, flags cleared;
//   7. the result is nInitialCorrespondences - nBad of the last round run;
//   8. a round without active edges runs no iteration (SparseOptimizer::optimize returns at once: no vertex is active);
//   9. information() * _error is the full matrix product, zeros included: a non-finite error row makes the chi2 NaN, and NaN
//      is not `> threshold`, so such an edge counts as an inlier.
//
// Summation order: csrc/lm_math.h's (edge k on lane k mod 256, ascending k, the fixed tree), for the 21 + 6 entries of H and b
// and for every chi2 sum.  Edges on level 1 (outliers) are SKIPPED: a lane's partial sum does not see them.
#pragma once
#include "lm_math.h"

namespace rgbl {

constexpr int kPoLanes = kLmLanes;
constexpr int kPoRegEdges = 8;     // edges a lane keeps in registers
constexpr int kPoRounds = 4;       // Optimizer.cc:1006
constexpr int kPoIterations = 10;  // its[] (:1003)
constexpr int kPoSums = LmSystem<6>::kSums;   // 28: upper triangle of H (21), b (6), the robust chi2 (1)

// ---- sin / cos -------------------------------------------------------------------------------------------------------
// fdlibm's __kernel_sin / __kernel_cos (the msun forms) on [-pi/4, pi/4] with a tail y
RGBL_HD double po_ksin(double x, double y) {
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double z = x * x, v = z * x, r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
RGBL_HD double po_kcos(double x, double y) {
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double z = x * x, w = z * z, r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z, a = 1.0 - hz;
  return a + (((1.0 - a) - hz) + (z * r - x * y));
}
// x = n * pi/2 + (y0 + y1), |y0| <= pi/4 (+ rounding); pi/2 = pio2_1 (33 bits) + pio2_1t; n * pio2_1 is exact for |n| < 2^20
RGBL_HD int po_rem_pio2(double x, double* y0, double* y1) {
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
  const double fn = rint(x * invpio2);
  const double r = x - fn * pio2_1, w = fn * pio2_1t;
  *y0 = r - w;
  *y1 = (r - *y0) - w;
  return (int)fn;
}
RGBL_HD double po_sin(double x) {
  if (!(fabs(x) <= 1048576.0)) return (x - x) / 0.0;   // NaN
  double y0, y1;
  const int n = po_rem_pio2(x, &y0, &y1) & 3;
  const double s = (n & 1) ? po_kcos(y0, y1) : po_ksin(y0, y1);
  return (n & 2) ? -s : s;
}
RGBL_HD double po_cos(double x) {
  if (!(fabs(x) <= 1048576.0)) return (x - x) / 0.0;
  double y0, y1;
  const int n = po_rem_pio2(x, &y0, &y1) & 3;
  const double c = (n & 1) ? po_ksin(y0, y1) : po_kcos(y0, y1);
  return (n == 1 || n == 2) ? -c : c;
}

// ---- SE3Quat -----------------------------------------------------------------------------------------------------------
struct PoPose { double q[4], t[3]; };   // q = x, y, z, w (Eigen's coeffs order)
struct PoCam { double fx, fy, cx, cy, bf; };

// SE3Quat::normalizeRotation (se3quat.h:280-285); Eigen's normalize() divides by the norm when the squared norm is > 0
RGBL_HD void po_normalize_rotation(double q[4]) {
  if (q[3] < 0.0) { q[0] *= -1.0; q[1] *= -1.0; q[2] *= -1.0; q[3] *= -1.0; }
  const double z = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (z > 0.0) {
    const double nrm = sqrt(z);
    q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
  }
}
// SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>()) (Optimizer.cc:831, se3quat.h:62-64)
RGBL_HD PoPose po_pose_from_float(const float q[4], const float t[3]) {
  PoPose T;
  for (int i = 0; i < 4; ++i) T.q[i] = (double)q[i];
  for (int i = 0; i < 3; ++i) T.t[i] = (double)t[i];
  po_normalize_rotation(T.q);
  return T;
}
// Quaternion * vector as Eigen's _transformVector: uv = vec x v; uv += uv; v + w uv + vec x uv
RGBL_HD void po_rotate(const double q[4], const double v[3], double r[3]) {
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  r[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
  r[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
  r[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}
// SE3Quat::map (se3quat.h:217-220): _r * xyz + _t
RGBL_HD void po_map(const PoPose& T, const double X[3], double P[3]) {
  po_rotate(T.q, X, P);
  P[0] = P[0] + T.t[0]; P[1] = P[1] + T.t[1]; P[2] = P[2] + T.t[2];
}
// Quaterniond(Matrix3d) as Eigen assigns it (Geometry/Quaternion.h); m is row-major
RGBL_HD void po_quat_from_matrix(const double m[9], double q[4]) {
  double t = (m[0] + m[4]) + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else if (!(m[4] > m[0]) && !(m[8] > m[0])) {   // i = 0, j = 1, k = 2
    t = sqrt(((m[0] - m[4]) - m[8]) + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[7] - m[5]) * t;
    q[1] = (m[3] + m[1]) * t;
    q[2] = (m[6] + m[2]) * t;
  } else if (m[4] > m[0] && !(m[8] > m[4])) {      // i = 1, j = 2, k = 0
    t = sqrt(((m[4] - m[8]) - m[0]) + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[2] - m[6]) * t;
    q[2] = (m[7] + m[5]) * t;
    q[0] = (m[1] + m[3]) * t;
  } else {                                         // i = 2, j = 0, k = 1
    t = sqrt(((m[8] - m[0]) - m[4]) + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[3] - m[1]) * t;
    q[0] = (m[2] + m[6]) * t;
    q[1] = (m[5] + m[7]) * t;
  }
}
// VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:73-76): SE3Quat::exp(update) * estimate, with SE3Quat::exp as written
// (se3quat.h:223-257, its theta < 1e-5 branch included), operator* (:104-110) and normalizeRotation.
// update = (omega, upsilon)
RGBL_HD PoPose po_oplus(const double u[6], const PoPose& T) {
  const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double O[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};   // skew(omega), se3_ops.hpp
  double O2[9], R[9], V[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) O2[3 * r + c] = (O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c]) + O[3 * r + 2] * O[6 + c];
  if (theta < 0.00001) {
    for (int i = 0; i < 9; ++i) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i]; V[i] = R[i]; }
  } else {
    const double s = po_sin(theta), c = po_cos(theta), t2 = theta * theta;
    const double a = s / theta, b = (1.0 - c) / t2, d = (theta - s) / (t2 * theta);
    for (int i = 0; i < 9; ++i) {
      const double I = i % 4 == 0 ? 1.0 : 0.0;
      R[i] = (I + a * O[i]) + b * O2[i];
      V[i] = (I + b * O[i]) + d * O2[i];
    }
  }
  PoPose E, N;
  po_quat_from_matrix(R, E.q);
  for (int r = 0; r < 3; ++r) E.t[r] = (V[3 * r] * u[3] + V[3 * r + 1] * u[4]) + V[3 * r + 2] * u[5];
  po_normalize_rotation(E.q);   // the SE3Quat(Quaterniond, Vector3d) constructor
  double rt[3];
  po_rotate(E.q, T.t, rt);
  for (int r = 0; r < 3; ++r) N.t[r] = E.t[r] + rt[r];
  const double* a = E.q; const double* b = T.q;   // Eigen's quaternion product
  N.q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
  N.q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
  N.q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
  N.q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
  po_normalize_rotation(N.q);
  return N;
}

// ---- edges ---------------------------------------------------------------------------------------------------------------
// One correspondence.  Xw, the observation and invSigma2 are the reference's floats (cast to double where they are used: exact).
struct PoEdge {
  float Xw[3], obs[3], info;   // obs[2] = mvuRight (>= 0: a stereo edge, Optimizer.cc:866)
  uint8_t stereo, level;       // level 1: an outlier, left out of the next optimisation (e->setLevel(1))
  double chi2;                 // e->chi2() of the error computed last
};

RGBL_HD double po_delta(bool stereo) { return (double)(float)sqrt(stereo ? 7.815 : 5.991); }   // Optimizer.cc:852-853, float

// computeError() and chi2() (base_edge.h:60): the edge's error at pose T, and _error.dot(information() * _error) with the
// full diagonal matrix product (quirk 9).  P = the mapped point.
RGBL_HD double po_edge_error(const PoEdge& e, const PoCam& C, const PoPose& T, double P[3], double err[3]) {
  const double X[3] = {(double)e.Xw[0], (double)e.Xw[1], (double)e.Xw[2]};
  po_map(T, X, P);
  const double s = (double)e.info;
  if (e.stereo) {
    // EdgeStereoSE3ProjectXYZOnlyPose::cam_project (types_six_dof_expmap.cpp:339-346): invz is a FLOAT
    const double invz = (double)(float)(1.0 / P[2]);
    const double u = P[0] * invz * C.fx + C.cx, v = P[1] * invz * C.fy + C.cy;
    err[0] = (double)e.obs[0] - u;
    err[1] = (double)e.obs[1] - v;
    err[2] = (double)e.obs[2] - (u - C.bf * invz);
    const double w0 = (s * err[0] + 0.0 * err[1]) + 0.0 * err[2], w1 = (0.0 * err[0] + s * err[1]) + 0.0 * err[2],
                 w2 = (0.0 * err[0] + 0.0 * err[1]) + s * err[2];
    return (err[0] * w0 + err[1] * w1) + err[2] * w2;
  }
  // EdgeSE3ProjectXYZOnlyPose::computeError, Pinhole::project (Pinhole.cpp:35-41): float parameters promoted
  err[0] = (double)e.obs[0] - (C.fx * P[0] / P[2] + C.cx);
  err[1] = (double)e.obs[1] - (C.fy * P[1] / P[2] + C.cy);
  err[2] = 0.0;
  const double w0 = s * err[0] + 0.0 * err[1], w1 = 0.0 * err[0] + s * err[1];
  return err[0] * w0 + err[1] * w1;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
RGBL_HD void po_huber(double e, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) { *rho0 = e; *rho1 = 1.0; return; }
  const double sqrte = sqrt(e);
  *rho0 = 2.0 * sqrte * delta - dsqr;
  *rho1 = delta / sqrte;
}

// the robust chi2 of one edge as SparseOptimizer::activeRobustChi2 adds it (sparse_optimizer.cpp:100-114)
RGBL_HD double po_edge_rho(const PoEdge& e, bool robust) {
  if (!robust) return e.chi2;
  double r0, r1;
  po_huber(e.chi2, po_delta(e.stereo != 0), &r0, &r1);
  return r0;
}

// linearizeOplus + constructQuadraticForm (base_unary_edge.hpp:43-72) of one active edge at pose T, added to a lane's partial
// sums acc[28]: H's upper triangle row by row (21), b (6), the robust chi2.  The information is scaled by rho[1] only
// (base_edge.h:96-102).  Also stores the edge's chi2.
RGBL_HD void po_edge_accumulate(PoEdge& e, const PoCam& C, const PoPose& T, bool robust, double acc[kPoSums]) {
  double P[3], err[3], A[3][6];
  e.chi2 = po_edge_error(e, C, T, P, err);
  double rho0 = e.chi2, rho1 = 1.0;
  if (robust) po_huber(e.chi2, po_delta(e.stereo != 0), &rho0, &rho1);
  const double x = P[0], y = P[1], z = P[2];
  if (e.stereo) {   // types_six_dof_expmap.cpp:375-404, the double invz
    const double invz = 1.0 / z, invz_2 = invz * invz;
    A[0][0] = x * y * invz_2 * C.fx;
    A[0][1] = -(1.0 + (x * x * invz_2)) * C.fx;
    A[0][2] = y * invz * C.fx;
    A[0][3] = -invz * C.fx;
    A[0][4] = 0.0;
    A[0][5] = x * invz_2 * C.fx;
    A[1][0] = (1.0 + y * y * invz_2) * C.fy;
    A[1][1] = -x * y * invz_2 * C.fy;
    A[1][2] = -x * invz * C.fy;
    A[1][3] = 0.0;
    A[1][4] = -invz * C.fy;
    A[1][5] = y * invz_2 * C.fy;
    A[2][0] = A[0][0] - C.bf * y * invz_2;
    A[2][1] = A[0][1] + C.bf * x * invz_2;
    A[2][2] = A[0][2];
    A[2][3] = A[0][3];
    A[2][4] = 0.0;
    A[2][5] = A[0][5] - C.bf * invz_2;
  } else {          // -projectJac * SE3deriv (OptimizableTypes.cpp:49-63, Pinhole.cpp:71-81): the full product
    const double J[2][3] = {{C.fx / z, 0.0, -C.fx * x / (z * z)}, {0.0, C.fy / z, -C.fy * y / (z * z)}};
    const double S[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 6; ++c) A[r][c] = -((J[r][0] * S[0][c] + J[r][1] * S[1][c]) + J[r][2] * S[2][c]);
    for (int c = 0; c < 6; ++c) A[2][c] = 0.0;
  }
  const int rows = e.stereo ? 3 : 2;
  const double s = (double)e.info, w = rho1 * s;   // weightedOmega = rho[1] * information
  const double oe[3] = {s * err[0], s * err[1], s * err[2]};   // omega * _error (the exact zeros of the diagonal matrix left out)
  int k = 0;
  for (int j = 0; j < 6; ++j)
    for (int c = j; c < 6; ++c, ++k) {
      double h = A[0][j] * (w * A[0][c]) + A[1][j] * (w * A[1][c]);
      if (rows == 3) h = h + A[2][j] * (w * A[2][c]);
      acc[k] = acc[k] + h;
    }
  for (int j = 0; j < 6; ++j) {
    double g = A[0][j] * oe[0] + A[1][j] * oe[1];
    if (rows == 3) g = g + A[2][j] * oe[2];
    acc[21 + j] = acc[21 + j] - rho1 * g;
  }
  acc[27] = acc[27] + rho0;
}

// what the tests compare besides pose, flags and count
struct PoDiag {
  int32_t iterations[kPoRounds];   // solve() calls of the round's optimize() (0: no active edge)
  int32_t active[kPoRounds];       // edges on level 0 when the round began
  double chi2[kPoRounds];          // the Levenberg currentChi when the round's optimize() returned (0 without iteration)
  int32_t rounds, reserved;        // rounds run (0: fewer than 3 correspondences)
  double q[4], t[3];               // the vertex estimate before :1109-1110 cast it to float (x y z w)
};

// ---- the four rounds -------------------------------------------------------------------------------------------------------
// The model lm_levenberg<6> runs: the vertex estimate and the two passes over the edges.
struct PoModel {
  const PoCam& C;
  PoPose T, Tt;   // the estimate, and the one of the trial (written by trial, read by accept)
  bool robust;
  RGBL_HD PoModel(const PoCam& cam, const PoPose& estimate, bool robust_kernel) : C(cam), T(estimate), robust(robust_kernel) {}
  template <class Lanes> RGBL_HD void linearise(Lanes& G) {
    G.zero();
    G.each([&](PoEdge& e, double* acc) { if (!e.level) po_edge_accumulate(e, C, T, robust, acc); });
  }
  template <class Lanes> RGBL_HD void trial(Lanes& G, const double* x) {
    Tt = po_oplus(x, T);
    G.zero();
    G.each([&](PoEdge& e, double* acc) {
      if (e.level) return;
      double P[3], err[3];
      e.chi2 = po_edge_error(e, C, Tt, P, err);
      acc[0] = acc[0] + po_edge_rho(e, robust);
    });
  }
  RGBL_HD void accept() { T = Tt; }
};

// Written once for both execution models.  `G` owns the problem's edges and the partial sums: the lanes of csrc/lm_math.h
// (zero, each, reduce_system, reduce_one) with kPoSums sums.  On the device every work-item runs this function; all scalar
// state is computed redundantly and identically by all of them, so the only synchronisation is inside G's reductions.  Every
// loop is bounded: 4 x 10 x 10 trials.
// Returns nInitialCorrespondences - nBad (:1113); `out` is the vertex estimate.
template <class Lanes>
RGBL_HD int po_optimize(Lanes& G, const PoCam& C, const PoPose& entry, int n_corr, PoPose& out, PoDiag& D) {
  for (int r = 0; r < kPoRounds; ++r) { D.iterations[r] = 0; D.active[r] = 0; D.chi2[r] = 0.0; }
  D.rounds = 0; D.reserved = 0;
  out = entry;
  for (int i = 0; i < 4; ++i) D.q[i] = entry.q[i];
  for (int i = 0; i < 3; ++i) D.t[i] = entry.t[i];
  if (n_corr < 3) return 0;   // :996-997
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int nBad = 0;
  for (int round = 0; round < kPoRounds; ++round) {
    PoModel M(C, entry, round < 3);   // quirk 1; quirk 4: setRobustKernel(0) at it == 2 acts from round 3 on
    const int n_active = n_corr - nBad;
    int iters = 0;
    double currentChi = 0.0;
    if (n_active > 0) {               // quirk 8
      // lm_levenberg<6>(G, M, kPoIterations, x, &iters, &currentChi) of csrc/lm_math.h WRITTEN OUT (comments there; a change
      // there belongs here too): called, the same loop costs k_pose_opt 0.3 - 0.7 % on the MI355X (docs/history/r15_measured.md)
      typedef LmSystem<6> Sys;
      double lambda = 0.0, ni = 2.0, sums[kPoSums];
      int lmBad = 0;
      for (int it = 0; it < kPoIterations; ++it) {
        M.linearise(G);
        const double* S = G.reduce_system(sums);
        currentChi = S[Sys::kChi];
        const double iniChi = currentChi;
        double tempChi = currentChi, rho = 0.0;
        int qmax = 0;
        if (it == 0) {
          double maxDiagonal = 0.0;
          for (int j = 0; j < 6; ++j) { const double a = fabs(S[Sys::diag(j)]); maxDiagonal = a > maxDiagonal ? a : maxDiagonal; }
          lambda = 1e-5 * maxDiagonal; ni = 2.0; lmBad = 0;
        }
        do {
          const bool ok = lm_solve<6>(S, lambda, S + Sys::kB, x);
          M.trial(G, x);
          tempChi = G.reduce_one();
          if (!ok) tempChi = DBL_MAX;
          rho = currentChi - tempChi;
          double scale = 0.0;
          for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + S[Sys::kB + j]);
          scale += 1e-3; rho /= scale;
          if (rho > 0.0 && tempChi >= -DBL_MAX && tempChi <= DBL_MAX) {
            const double c = 2.0 * rho - 1.0;
            double alpha = 1.0 - c * c * c;
            alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;
            const double scaleFactor = (1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0;
            lambda *= scaleFactor; ni = 2.0;
            currentChi = tempChi; M.accept();
          } else {
            lambda *= ni; ni *= 2.0;
          }
          ++qmax;
        } while (rho < 0.0 && qmax < kLmTrials);
        ++iters;
        if (qmax == kLmTrials || rho == 0.0) break;
        if ((iniChi - currentChi) * 1e3 < iniChi) ++lmBad; else lmBad = 0;
        if (lmBad >= 3) break;
      }
    }
    const PoPose& T = M.T;
    // Optimizer.cc:1014-1100
    G.zero();
    G.each([&](PoEdge& e, double* acc) {
      if (e.level) {
        double P[3], err[3];
        e.chi2 = po_edge_error(e, C, T, P, err);
      }
      const float chi2 = (float)e.chi2;   // quirk 3
      e.level = chi2 > (e.stereo ? 7.815f : 5.991f) ? 1 : 0;
      acc[0] = acc[0] + (double)e.level;
    });
    nBad = (int)G.reduce_one();
    D.iterations[round] = iters; D.active[round] = n_active; D.chi2[round] = currentChi;
    D.rounds = round + 1;
    out = T;
    for (int i = 0; i < 4; ++i) D.q[i] = T.q[i];
    for (int i = 0; i < 3; ++i) D.t[i] = T.t[i];
    if (n_corr < 10) break;   // quirk 5
  }
  return n_corr - nBad;
}

}  // namespace rgbl
