// mlpnp_math.h — MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp) for pinhole cameras without covariance information
// (covs(1), use_cov == false, as iterate and Refine call computePose), in ONE place for host and device: the constructor's
// bookkeeping (:55-97), computePose (:356-658), rot2rodrigues / rodrigues2rot (:660-692), mlpnp_gn (:694-758), the residuals
// (:760-806), CheckInliers (:262-293) and the stop rule of iterate + Refine (:100-223, :295-353) as a scan over the counts.
//
// Arithmetic.  fp64 where the reference is fp64 (everything inside computePose), fp32 where it is fp32: the bearing
// ((u - cx) / fx, (v - cy) / fy, 1) - NOT normalised, the reference's comment is wrong and its code counts -, mvMaxError =
// sigma2 * th2, the camera-frame point of CheckInliers (double-times-float products summed in double, rounded to float),
// Pinhole::project and the squared error.  No contraction (-ffp-contract=off); division and square root are IEEE on host and
// device.  Host build, emulated kernels and MI355X agree bit for bit, NaN cases included.
//
// What IS pinned: the branch structure of computePose (the planarity test on the UNCENTRED sum of p p^T - rank 2 means a plane
// through the world origin - with Eigen's full-pivot Householder rank rule |R_kk| > max pivot * 3 * DBL_EPSILON; rank 2 takes
// the 9-column branch, every other rank the 12-column one; a matrix with a non-finite entry counts as rank 0, where Eigen's
// pivot search leaves the order open), the design matrix, the scale (cube root / square root), the det < 0
// flips, the translation sign tests over the FIRST SIX correspondences of the set (two-way / four-way, first minimum), the
// `> epsilon` guards of both Rodrigues functions (acos of an argument past 1 gives NaN, which fails the guard), Gauss-Newton on
// the UNROTATED points in the planar branch too, at most 5 iterations, the `max|dx| > 5 || min|dx| > 1` break before the update
// and the `max|J dx| < 1e-5` stop after it, CheckInliers without a depth-sign test (NaN is an outlier), and the stop rule.
//
// What is NOT pinned - the header owns it:
//   - the two null-space vectors of a bearing f = (x, y, 1): r = (0, -1, y) / |.|, s = f x r / |.| (the reference takes them from a
//     JacobiSVD; the result is invariant to the basis up to rounding);
//   - the eigenvector of the smallest eigenvalue of A^T A (the reference: JacobiSVD, last column of V): a fixed-sweep cyclic
//     Jacobi in fp64 in the round-robin (tournament) order, kMlSweeps sweeps, no data-dependent exit; the rotations of one step
//     are disjoint and are spread over the lanes in three phases (angles; columns of A and V; rows of A) - the host runs the
//     same phases in the same order; the first smallest diagonal entry wins;
//   - the 3 x 3 eigen frame (SelfAdjointEigenSolver): Jacobi, ascending, each vector's largest entry positive;
//   - the nearest rotation U V^T (JacobiSVD of the 3 x 3): V and the singular values from Jacobi on M^T M, u_i = M v_i / |M v_i|
//     for the two largest, the third by the cross product with the sign that det M and det V give;
//   - Ts[s].inverse() of a rigid transformation, written as (R^T, -R^T t);
//   - sin / cos (po_sin, po_cos), acos as atan2(sqrt((1 - x)(1 + x)), x) with s3_atan2, pow(x, 1/3) as a Newton cube root;
//   - Eigen's LDLT, replaced by lm_solve<6> with lambda = 0, and the order of Eigen's small products (left to right);
//   - the Jacobian: derived here from d/dw, d/dt of n^T normalize(R(w) X + t) with R = I + a K + b K^2, a = sin|w| / |w|,
//     b = (1 - cos|w|) / |w|^2; the reference's generated expressions (mlpnpJacs) are not transcribed.  Its singularity at
//     w = 0 is kept: w_k / |w| is 0 / 0 there, the Jacobian is NaN, the solve fails, x stays.
//
// Deliberate deviation (undefined in the reference): a dx with a non-finite entry, and a failed lm_solve, end the Gauss-Newton
// loop as the break rule does, with x unchanged.
//
// Summation order.  Every sum over the six correspondences of a sample (the 6 entries of the planarity matrix, the 78 / 45 of
// A^T A, the 21 + 6 of the normal equations) uses csrc/lm_math.h's order for six lanes: partial sums 0.0 + term on lanes
// 0 .. 5, every other lane +0.0, the fixed tree - ml_sum6.
//
// Refine (:295-353).  As compiled, the reference discards the pose Refine computes (see ml_scan at the end of this file): what
// iterate returns after a "successful Refine" is the current hypothesis.  The code counts, so no set larger than six is ever
// solved here.
#pragma once
#include "lm_math.h"
#include "frustum_math.h"
#include "poseopt_math.h"
#include "sim3_math.h"

namespace rgbl {

constexpr int kMlSweeps = 12;      // round-robin Jacobi sweeps of the 12 x 12 / 9 x 9: chosen with a margin; the smallest count that
                                   // keeps the model comparison of tests/test_mlpnp_math.py has not been looked for
constexpr int kMl3Sweeps = 8;      // of the 3 x 3 matrices
constexpr int kMlGnSums = 27;      // upper triangle of J^T J row by row (21), J^T r (6)
constexpr int kMlGnIterations = 5; // maxIt (:718)

// one problem as the arithmetic reads it (host arrays or device arrays)
struct MlView {
  const float* xy;        // mvKeysUn, per feature
  const int32_t* oct;     // per feature
  const float* wpos;      // world positions, rows of 3
  const float* sigma2;    // mvLevelSigma2
  const int32_t* feat;    // per correspondence: mvKeyPointIndices
  const int32_t* point;   // per correspondence: row of wpos
  int N, n_levels;
  float K[4], th2;
};

// ---- the constructor's bookkeeping (:72-86) ------------------------------------------------------------------------------------
RGBL_HD void ml_corr(const MlView& v, int i, double f[3], double X[3]) {
  const int ft = v.feat[i];
  const size_t p = (size_t)v.point[i];
  f[0] = (double)fr_quot(v.xy[2 * (size_t)ft] - v.K[2], v.K[0]);       // Pinhole::unproject; `/= cv_br.z` divides by 1.f
  f[1] = (double)fr_quot(v.xy[2 * (size_t)ft + 1] - v.K[3], v.K[1]);
  f[2] = 1.0;
  X[0] = (double)v.wpos[3 * p]; X[1] = (double)v.wpos[3 * p + 1]; X[2] = (double)v.wpos[3 * p + 2];
}
RGBL_HD float ml_max_error(const MlView& v, int i) {
  const int oc = v.oct[v.feat[i]], o = oc < 0 ? 0 : (oc >= v.n_levels ? v.n_levels - 1 : oc);   // host arrays are checked before
  return v.sigma2[o] * v.th2;
}

// ---- small vector helpers --------------------------------------------------------------------------------------------------------
RGBL_HD double ml_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
RGBL_HD double ml_norm(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
RGBL_HD void ml_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
RGBL_HD void ml_matvec(const double* R, const double* x, double* y) {   // row-major 3 x 3
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
}
RGBL_HD double ml_det3(const double* R) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}
RGBL_HD bool ml_finite(double x) { return x >= -DBL_MAX && x <= DBL_MAX; }

// the null space of f = (x, y, 1)
RGBL_HD void ml_nullspace(const double* f, double* r, double* s) {
  const double nr = sqrt(1.0 + f[1] * f[1]);
  r[0] = 0.0; r[1] = -1.0 / nr; r[2] = f[1] / nr;
  double c[3];
  ml_cross(f, r, c);
  const double ns = ml_norm(c);
  s[0] = c[0] / ns; s[1] = c[1] / ns; s[2] = c[2] / ns;
}

// the fixed tree of lm_math.h over six partial sums on lanes 0 .. 5 (every other lane holds +0.0)
RGBL_HD double ml_sum6(double v0, double v1, double v2, double v3, double v4, double v5) {
  v0 = v0 + 0.0; v1 = v1 + 0.0; v2 = v2 + 0.0; v3 = v3 + 0.0; v4 = v4 + 0.0; v5 = v5 + 0.0;   // s = 128 .. 8
  const double a0 = v0 + v4, a1 = v1 + v5, a2 = v2 + 0.0, a3 = v3 + 0.0;                       // s = 4
  return (a0 + a2) + (a1 + a3);                                                                 // s = 2, 1
}

// the cube root of a positive number (pow(x, 1.0 / 3.0) in the reference): bit estimate, six Newton steps
RGBL_HD double ml_cbrt(double x) {
  if (!(x > 0.0) || !(x <= DBL_MAX)) return x;   // 0, NaN, inf
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  u = u / 3 + 0x2A9F7893782DA1CEull;
  double y;
  __builtin_memcpy(&y, &u, 8);
#pragma unroll 1
  for (int i = 0; i < 6; ++i) y = y - (y * y * y - x) / (3.0 * (y * y));
  return y;
}
RGBL_HD double ml_acos(double x) { return s3_atan2(sqrt((1.0 - x) * (1.0 + x)), x); }

// ---- Jacobi on small symmetric matrices in registers ------------------------------------------------------------------------------
RGBL_HD void ml_jacobi_cs(double app, double aqq, double apq, double* c, double* s, double* t) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  *t = apq == 0.0 ? 0.0 : tt;
  *c = 1.0 / sqrt(*t * *t + 1.0);
  *s = *t * *c;
}
template <int P, int Q> RGBL_HD void ml_rotate3(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  double c, s, t;
  ml_jacobi_cs(a[P][P], a[Q][Q], apq, &c, &s, &t);
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
  constexpr int r = 3 - P - Q;
  const double arp = a[r][P], arq = a[r][Q];
  a[r][P] = c * arp - s * arq;
  a[r][Q] = s * arp + c * arq;
  a[P][r] = a[r][P];
  a[Q][r] = a[r][Q];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vp = v[i][P], vq = v[i][Q];
    v[i][P] = c * vp - s * vq;
    v[i][Q] = s * vp + c * vq;
  }
}
template <int I, int J> RGBL_HD void ml_swap_cols(bool doit, double (&e)[3], double (&v)[3][3]) {
  const double ei = e[I], ej = e[J];
  e[I] = doit ? ej : ei; e[J] = doit ? ei : ej;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double vi = v[r][I], vj = v[r][J];
    v[r][I] = doit ? vj : vi; v[r][J] = doit ? vi : vj;
  }
}
// eigenvalues ascending (descending: largest first), eigenvectors in the columns of v; m: xx xy xz yy yz zz
RGBL_HD void ml_eig3(const double* m, bool descending, double (&e)[3], double (&v)[3][3]) {
  double a[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kMl3Sweeps; ++sweep) {
    ml_rotate3<0, 1>(a, v);
    ml_rotate3<0, 2>(a, v);
    ml_rotate3<1, 2>(a, v);
  }
  e[0] = a[0][0]; e[1] = a[1][1]; e[2] = a[2][2];
  ml_swap_cols<0, 1>(descending ? e[1] > e[0] : e[1] < e[0], e, v);
  ml_swap_cols<1, 2>(descending ? e[2] > e[1] : e[2] < e[1], e, v);
  ml_swap_cols<0, 1>(descending ? e[1] > e[0] : e[1] < e[0], e, v);
}

// rank of the symmetric 3 x 3 as Eigen::FullPivHouseholderQR::rank() counts it with the default threshold
RGBL_HD int ml_rank3(const double* m) {
  double a[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
  double diag[3], maxpivot = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int bi = k, bj = k;
    double big = -1.0;
#pragma unroll
    for (int j = k; j < 3; ++j) {
#pragma unroll
      for (int i = k; i < 3; ++i) {
        const double v = fabs(a[i][j]);
        if (v > big) { big = v; bi = i; bj = j; }
      }
    }
    if (big > maxpivot) maxpivot = big;
#pragma unroll
    for (int i = k + 1; i < 3; ++i) {
      const bool sw = bi == i;
#pragma unroll
      for (int j = 0; j < 3; ++j) { const double x = a[k][j], y = a[i][j]; a[k][j] = sw ? y : x; a[i][j] = sw ? x : y; }
    }
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      const bool sw = bj == j;
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double x = a[i][k], y = a[i][j]; a[i][k] = sw ? y : x; a[i][j] = sw ? x : y; }
    }
    double tail2 = 0.0;
#pragma unroll
    for (int i = k + 1; i < 3; ++i) tail2 += a[i][k] * a[i][k];
    const double c0 = a[k][k];
    double beta = c0, tau = 0.0, vv[3] = {0.0, 0.0, 0.0};
    if (tail2 > DBL_MIN) {   // makeHouseholder
      beta = sqrt(c0 * c0 + tail2);
      if (c0 >= 0.0) beta = -beta;
#pragma unroll
      for (int i = k + 1; i < 3; ++i) vv[i] = a[i][k] / (c0 - beta);
      tau = (beta - c0) / beta;
    }
    diag[k] = beta;
#pragma unroll
    for (int j = k + 1; j < 3; ++j) {
      double w = a[k][j];
#pragma unroll
      for (int i = k + 1; i < 3; ++i) w += vv[i] * a[i][j];
      a[k][j] = a[k][j] - tau * w;
#pragma unroll
      for (int i = k + 1; i < 3; ++i) a[i][j] = a[i][j] - tau * w * vv[i];
    }
  }
  const double thr = maxpivot * (3.0 * DBL_EPSILON);
  bool finite = true;   // a matrix with a non-finite entry has rank 0 here (Eigen's maxCoeff leaves the pivot order open then)
#pragma unroll
  for (int i = 0; i < 6; ++i) finite = finite && ml_finite(m[i]);
  if (!finite) return 0;
  int rank = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) rank += fabs(diag[k]) > thr ? 1 : 0;
  return rank;
}

// the rows of SelfAdjointEigenSolver(planarTest).eigenvectors().transpose() (:394-396), row-major
RGBL_HD void ml_eigen_frame(const double* m, double* E) {
  double e[3], v[3][3];
  ml_eig3(m, false, e, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double a0 = fabs(v[0][c]), a1 = fabs(v[1][c]), a2 = fabs(v[2][c]);
    const double top = (a0 >= a1 && a0 >= a2) ? v[0][c] : (a1 >= a2 ? v[1][c] : v[2][c]);
    const double sg = top < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) E[3 * c + r] = sg * v[r][c];
  }
}

// U V^T of the SVD of M (row-major)
RGBL_HD void ml_nearest_rotation(const double* M, double* R) {
  double b[6];   // M^T M
  b[0] = M[0] * M[0] + M[3] * M[3] + M[6] * M[6];
  b[1] = M[0] * M[1] + M[3] * M[4] + M[6] * M[7];
  b[2] = M[0] * M[2] + M[3] * M[5] + M[6] * M[8];
  b[3] = M[1] * M[1] + M[4] * M[4] + M[7] * M[7];
  b[4] = M[1] * M[2] + M[4] * M[5] + M[7] * M[8];
  b[5] = M[2] * M[2] + M[5] * M[5] + M[8] * M[8];
  double e[3], v[3][3];
  ml_eig3(b, true, e, v);
  double U[3][3];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double vc[3] = {v[0][c], v[1][c], v[2][c]};
    double w[3];
    ml_matvec(M, vc, w);
    const double n = ml_norm(w);
    U[0][c] = w[0] / n; U[1][c] = w[1] / n; U[2][c] = w[2] / n;
  }
  const double V9[9] = {v[0][0], v[0][1], v[0][2], v[1][0], v[1][1], v[1][2], v[2][0], v[2][1], v[2][2]};
  const double sg = (ml_det3(V9) < 0.0 ? -1.0 : 1.0) * (ml_det3(M) < 0.0 ? -1.0 : 1.0);
  const double u0[3] = {U[0][0], U[1][0], U[2][0]}, u1[3] = {U[0][1], U[1][1], U[2][1]};
  double u2[3];
  ml_cross(u0, u1, u2);
  U[0][2] = sg * u2[0]; U[1][2] = sg * u2[1]; U[2][2] = sg * u2[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[i][0] * v[j][0] + U[i][1] * v[j][1] + U[i][2] * v[j][2];
  }
}

// ---- rodrigues2rot (:660-675), rot2rodrigues (:677-692) ---------------------------------------------------------------------------
RGBL_HD void ml_rodrigues2rot(const double* w, double* R) {
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  const double n = ml_norm(w);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (n > DBL_EPSILON) {
    const double a = po_sin(n) / n, b = (1.0 - po_cos(n)) / (n * n);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double k2 = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
        R[3 * i + j] = (R[3 * i + j] + a * K[3 * i + j]) + b * k2;
      }
    }
  }
}
RGBL_HD void ml_rot2rodrigues(const double* R, double* w) {
  w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
  const double trace = (R[0] + R[4] + R[8]) - 1.0;
  const double wnorm = ml_acos(trace / 2.0);
  if (wnorm > DBL_EPSILON) {
    const double sc = wnorm / (2.0 * po_sin(wnorm));
    w[0] = (R[7] - R[5]) * sc; w[1] = (R[2] - R[6]) * sc; w[2] = (R[3] - R[1]) * sc;
  }
}

// ---- the execution ----------------------------------------------------------------------------------------------------------------
// X, the lanes that run one computePose together: x.lane, x.lanes, x.sync() (orders the work space between phases), x.all(p)
// (p of every lane).  The host is one lane that runs every phase's loop to its end.  Whatever is not inside a
// `for (.. = x.lane; ..; .. += x.lanes)` loop is computed redundantly and identically by every lane.
struct MlHostX {
  int lane = 0, lanes = 1;
  void sync() {}
  bool all(bool p) { return p; }
};
// the work space of one computePose: LDS on the device
struct MlWork {
  double A[12][12], V[12][12];
  double cs[6][2];
  double sums[78];             // the sums of a set: planarity (6), A^T A (78 / 45), normal equations (27)
  double row[6][2][12];        // a six-point set: its rows of A, then its rows of J (6) and r (1)
};

// round-robin pairing: `ring` + 1 players, player `ring` stays; pair k of step `step`, p < q
RGBL_HD void ml_pair(int k, int step, int ring, int* p, int* q) {
  int a, b;
  if (k == 0) { a = step; b = ring; }
  else { a = (step + k) % ring; b = (step - k + ring) % ring; }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}
RGBL_HD void ml_tri(int e, int n, int* i, int* j) {   // entry e of the upper triangle row by row
  int r = 0;
  while (e >= n - r) { e -= n - r; ++r; }
  *i = r; *j = r + e;
}

// W.sums[0 .. n (n + 1) / 2) -> the symmetric W.A, W.V = I; then the Jacobi; returns the column of W.V of the smallest diagonal entry
template <class X> RGBL_HD int ml_smallest_eigenvector(X& x, MlWork& W, int n) {
  const int ne = n * (n + 1) / 2;
  for (int e = x.lane; e < ne; e += x.lanes) {
    int i, j;
    ml_tri(e, n, &i, &j);
    W.A[i][j] = W.sums[e];
    W.A[j][i] = W.sums[e];
    W.V[i][j] = i == j ? 1.0 : 0.0;
    W.V[j][i] = i == j ? 1.0 : 0.0;
  }
  x.sync();
  const int players = n + (n & 1), half = players / 2, ring = players - 1;
  for (int sweep = 0; sweep < kMlSweeps; ++sweep) {
    for (int step = 0; step < ring; ++step) {
      for (int k = x.lane; k < half; k += x.lanes) {       // phase 1: the angles
        int p, q;
        ml_pair(k, step, ring, &p, &q);
        double c = 1.0, s = 0.0, t = 0.0;
        if (q < n) ml_jacobi_cs(W.A[p][p], W.A[q][q], W.A[p][q], &c, &s, &t);
        W.cs[k][0] = c; W.cs[k][1] = s;
      }
      x.sync();
      for (int w = x.lane; w < n * half; w += x.lanes) {   // phase 2: A <- A J, V <- V J
        const int r = w / half, k = w % half;
        int p, q;
        ml_pair(k, step, ring, &p, &q);
        if (q >= n) continue;
        const double c = W.cs[k][0], s = W.cs[k][1];
        const double arp = W.A[r][p], arq = W.A[r][q], vrp = W.V[r][p], vrq = W.V[r][q];
        W.A[r][p] = c * arp - s * arq; W.A[r][q] = s * arp + c * arq;
        W.V[r][p] = c * vrp - s * vrq; W.V[r][q] = s * vrp + c * vrq;
      }
      x.sync();
      for (int w = x.lane; w < n * half; w += x.lanes) {   // phase 3: A <- J^T A
        const int r = w / half, k = w % half;
        int p, q;
        ml_pair(k, step, ring, &p, &q);
        if (q >= n) continue;
        const double c = W.cs[k][0], s = W.cs[k][1];
        const double apr = W.A[p][r], aqr = W.A[q][r];
        W.A[p][r] = c * apr - s * aqr; W.A[q][r] = s * apr + c * aqr;
      }
      x.sync();
    }
  }
  int idx = 0;
  double low = W.A[0][0];
  for (int i = 1; i < n; ++i)
    if (W.A[i][i] < low) { low = W.A[i][i]; idx = i; }
  return idx;
}

// the two rows of A of one correspondence (:439-512): 12 entries, or 9 in the planar branch (pt = eigenRot * p)
RGBL_HD void ml_rows(const double* f, const double* pt, bool planar, double* rr, double* rs) {
  double r[3], s[3];
  ml_nullspace(f, r, s);
  // both branches' entries side by side and a select: written with `if (planar)` around two loops the compiler merges the two
  // sets of stores through a private array indexed at run time (24 bytes of scratch)
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    const double nr = c < 9 ? r[c < 9 ? c / 3 : 0] * pt[c % 3] : r[c < 9 ? 0 : c - 9];
    const double ns = c < 9 ? s[c < 9 ? c / 3 : 0] * pt[c % 3] : s[c < 9 ? 0 : c - 9];
    const double pr = c < 6 ? r[c < 6 ? c / 2 : 0] * pt[1 + c % 2] : (c < 9 ? r[c >= 6 && c < 9 ? c - 6 : 0] : 0.0);
    const double ps = c < 6 ? s[c < 6 ? c / 2 : 0] * pt[1 + c % 2] : (c < 9 ? s[c >= 6 && c < 9 ? c - 6 : 0] : 0.0);
    rr[c] = planar ? pr : nr;
    rs[c] = planar ? ps : ns;
  }
}
// ---- Gauss-Newton (:694-806) --------------------------------------------------------------------------------------------------
struct MlGn {
  double w[3], T[3], R[9];
  double a, b, c1[3], c2[3];   // sin t / t, (1 - cos t) / t^2, and their derivatives times w_k / t
};
RGBL_HD void ml_gn_state(const double* x, MlGn& G) {
#pragma unroll
  for (int i = 0; i < 3; ++i) { G.w[i] = x[i]; G.T[i] = x[3 + i]; }
  ml_rodrigues2rot(G.w, G.R);
  const double t = ml_norm(G.w), sn = po_sin(t), cn = po_cos(t);
  G.a = sn / t;
  G.b = (1.0 - cn) / (t * t);
  const double da = (t * cn - sn) / (t * t), db = (t * sn - 2.0 * (1.0 - cn)) / (t * t * t);
#pragma unroll
  for (int k = 0; k < 3; ++k) { const double u = G.w[k] / t; G.c1[k] = da * u; G.c2[k] = db * u; }
}
// residuals r[2] and the rows J0, J1 of one correspondence
RGBL_HD void ml_gn_rows(const MlGn& G, const double* f, const double* X, double* res, double* J0, double* J1) {
  double nr[3], ns[3], v[3], g[3];
  ml_nullspace(f, nr, ns);
  ml_matvec(G.R, X, v);
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = v[i] + G.T[i];
  const double nv = ml_norm(v);
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = v[i] / nv;
  res[0] = ml_dot(nr, g);
  res[1] = ml_dot(ns, g);
  double m0[3], m1[3];   // n^T (I - g g^T) / |v|
#pragma unroll
  for (int i = 0; i < 3; ++i) { m0[i] = (nr[i] - res[0] * g[i]) / nv; m1[i] = (ns[i] - res[1] * g[i]) / nv; }
  double kx[3], kkx[3];
  ml_cross(G.w, X, kx);
  ml_cross(G.w, kx, kkx);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double ex[3], ekx[3], kex[3], dv[3];
    ml_cross(e, X, ex);
    ml_cross(e, kx, ekx);
    ml_cross(G.w, ex, kex);
#pragma unroll
    for (int i = 0; i < 3; ++i) dv[i] = ((G.c1[k] * kx[i] + G.a * ex[i]) + G.c2[k] * kkx[i]) + G.b * (ekx[i] + kex[i]);
    J0[k] = ml_dot(m0, dv);
    J1[k] = ml_dot(m1, dv);
    J0[3 + k] = m0[k];
    J1[3 + k] = m1[k];
  }
}
RGBL_HD bool ml_gn_below(const double* J0, const double* J1, const double* dx) {   // both |J dx| of a correspondence < epsP
  double d0 = 0.0, d1 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) { d0 = d0 + J0[i] * dx[i]; d1 = d1 + J1[i] * dx[i]; }
  return fabs(d0) < 1e-5 && fabs(d1) < 1e-5;
}

// ---- the set of one computePose ---------------------------------------------------------------------------------------------------
// list[0 .. m): the correspondences (indices into the view's 0 .. N-1) in the order computePose sees them: a sample as drawn.
// Its first six entries are the ones the sign tests read.
struct MlSet {
  const MlView* v;
  const int32_t* list;
  int m;
};
RGBL_HD void ml_set_corr(const MlSet S, int j, double* f, double* X) { ml_corr(*S.v, S.list[j], f, X); }

// The sums of a six-point set, for any X: lanes 0 .. 5 put their correspondence's values into W.row, then one lane per entry
// forms ml_sum6 over the partial sums 0.0 + term.
struct MlSixSums {
  template <class X, class Term> RGBL_HD void reduce(X& x, MlWork& W, int ne, Term term) {
    x.sync();
    for (int e = x.lane; e < ne; e += x.lanes)
      W.sums[e] = ml_sum6(0.0 + term(e, 0), 0.0 + term(e, 1), 0.0 + term(e, 2), 0.0 + term(e, 3), 0.0 + term(e, 4), 0.0 + term(e, 5));
    x.sync();
  }
  template <class X> RGBL_HD void planar(X& x, MlWork& W, const MlSet S) {
    for (int j = x.lane; j < 6; j += x.lanes) {
      double f[3], P[3];
      ml_set_corr(S, j, f, P);
      W.row[j][0][0] = P[0]; W.row[j][0][1] = P[1]; W.row[j][0][2] = P[2];
    }
    reduce(x, W, 6, [&](int e, int j) { int a, b; ml_tri(e, 3, &a, &b); return W.row[j][0][a] * W.row[j][0][b]; });
  }
  template <class X> RGBL_HD void ata(X& x, MlWork& W, const MlSet S, bool planar, const double* E) {
    for (int j = x.lane; j < 6; j += x.lanes) {
      double f[3], P[3], pt[3], rr[12], rs[12];
      ml_set_corr(S, j, f, P);
      ml_matvec(E, P, pt);
#pragma unroll
      for (int c = 0; c < 3; ++c) pt[c] = planar ? pt[c] : P[c];
      ml_rows(f, pt, planar, rr, rs);
#pragma unroll
      for (int c = 0; c < 12; ++c) { W.row[j][0][c] = rr[c]; W.row[j][1][c] = rs[c]; }
    }
    const int n = planar ? 9 : 12;
    reduce(x, W, n * (n + 1) / 2, [&](int e, int j) {
      int a, b;
      ml_tri(e, n, &a, &b);
      return W.row[j][0][a] * W.row[j][0][b] + W.row[j][1][a] * W.row[j][1][b];
    });
  }
  template <class X> RGBL_HD void gn(X& x, MlWork& W, const MlSet S, const MlGn& G) {
    for (int j = x.lane; j < 6; j += x.lanes) {
      double f[3], P[3], res[2], J0[6], J1[6];
      ml_set_corr(S, j, f, P);
      ml_gn_rows(G, f, P, res, J0, J1);
#pragma unroll
      for (int c = 0; c < 6; ++c) { W.row[j][0][c] = J0[c]; W.row[j][1][c] = J1[c]; }
      W.row[j][0][6] = res[0]; W.row[j][1][6] = res[1];
    }
    reduce(x, W, kMlGnSums, [&](int e, int j) {
      int a = e - 21, b = 6;
      if (e < 21) ml_tri(e, 6, &a, &b);
      return W.row[j][0][a] * W.row[j][0][b] + W.row[j][1][a] * W.row[j][1][b];
    });
  }
  template <class X> RGBL_HD bool below(X& x, MlWork& W, const MlSet, const MlGn&, const double* dx) {
    bool ok = true;
    for (int j = x.lane; j < 6; j += x.lanes) ok = ml_gn_below(W.row[j][0], W.row[j][1], dx) && ok;
    return x.all(ok);
  }
};

// ---- computePose (:356-658) --------------------------------------------------------------------------------------------------------
// Q: the sums of the set (MlSixSums).  R (row-major) and t: `result`.  *gn_path (diagnostics):
// iterations that updated x, + 8 if the loop left at the break rule, + 16 at the stop rule, + 32 at a failed solve.
template <class X, class Sums>
RGBL_HD void ml_compute_pose(X& x, MlWork& W, Sums& Q, const MlSet S, double* R, double* t, int* gn_path) {
  x.sync();
  Q.planar(x, W, S);
  double pm[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) pm[i] = W.sums[i];
  const bool planar = ml_rank3(pm) == 2;
  double E[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if (planar) ml_eigen_frame(pm, E);
  Q.ata(x, W, S, planar, E);
  const int n = planar ? 9 : 12;
  const int col = ml_smallest_eigenvector(x, W, n);
  double r1[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) r1[i] = i < n ? W.V[i < n ? i : 0][col] : 0.0;
  double Rout[9], tout[3];
  if (planar) {
    const double c1[3] = {r1[0], r1[2], r1[4]}, c2[3] = {r1[1], r1[3], r1[5]};
    double c0[3];
    ml_cross(c1, c2, c0);
    const double Qm[9] = {c0[0], c0[1], c0[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]};
    const double q1[3] = {Qm[1], Qm[4], Qm[7]}, q2[3] = {Qm[2], Qm[5], Qm[8]};
    const double scale = 1.0 / sqrt(fabs(ml_norm(q1) * ml_norm(q2)));
    double R1[9];
    ml_nearest_rotation(Qm, R1);
    if (ml_det3(R1) < 0.0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
    }
    double B[9];   // eigenRot^T * Rout1
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) B[3 * i + j] = E[i] * R1[j] + E[3 + i] * R1[3 + j] + E[6 + i] * R1[6 + j];
    }
    const double tp[3] = {scale * r1[6], scale * r1[7], scale * r1[8]};
    double Ro[9];   // transposeInPlace, *= -1
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Ro[3 * i + j] = -B[3 * j + i];
    }
    if (ml_det3(Ro) < 0.0) { Ro[2] = -Ro[2]; Ro[5] = -Ro[5]; Ro[8] = -Ro[8]; }
    double R2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) { R2[3 * i] = -Ro[3 * i]; R2[3 * i + 1] = -Ro[3 * i + 1]; R2[3 * i + 2] = Ro[3 * i + 2]; }
    double val[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = 0; p < 6; ++p) {
      double f[3], P[3];
      ml_set_corr(S, p, f, P);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double v[3];
        ml_matvec(c < 2 ? Ro : R2, P, v);
        const double sg = (c & 1) ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = v[i] + sg * tp[i];
        const double nv = ml_norm(v);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = v[i] / nv;
        val[c] = val[c] + (1.0 - ml_dot(v, f));
      }
    }
    int idx = 0;   // std::min_element
    double low = val[0];
    if (val[1] < low) { low = val[1]; idx = 1; }
    if (val[2] < low) { low = val[2]; idx = 2; }
    if (val[3] < low) { low = val[3]; idx = 3; }
#pragma unroll
    for (int i = 0; i < 9; ++i) Rout[i] = idx < 2 ? Ro[i] : R2[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tout[i] = (idx & 1) ? -tp[i] : tp[i];
  } else {
    double tmp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) tmp[3 * i + j] = r1[3 * j + i];
    }
    const double n0 = ml_norm(r1), n1 = ml_norm(r1 + 3), n2 = ml_norm(r1 + 6);   // the columns of tmp
    const double scale = 1.0 / ml_cbrt(fabs(n0 * n1 * n2));
    double Rn[9];
    ml_nearest_rotation(tmp, Rn);
    if (ml_det3(Rn) < 0.0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rn[i] = -Rn[i];
    }
    const double ts[3] = {scale * r1[9], scale * r1[10], scale * r1[11]};
    double t0[3], Ri[9], ti[3];
    ml_matvec(Rn, ts, t0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Ri[3 * i + j] = Rn[3 * j + i];
    }
    ml_matvec(Ri, t0, ti);   // Ts[0].inverse() translates by -ti, Ts[1].inverse() by +ti
    double err[2] = {0.0, 0.0};
    for (int p = 0; p < 6; ++p) {
      double f[3], P[3], rp[3];
      ml_set_corr(S, p, f, P);
      ml_matvec(Ri, P, rp);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        double v[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = rp[i] + (s == 0 ? -ti[i] : ti[i]);
        const double nv = ml_norm(v);
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = v[i] / nv;
        err[s] = err[s] + (1.0 - ml_dot(v, f));
      }
    }
    const bool first = err[0] < err[1];
#pragma unroll
    for (int i = 0; i < 3; ++i) tout[i] = first ? -ti[i] : ti[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rout[i] = Ri[i];
  }
  // 5. gauss newton on the unrotated points
  double xg[6];
  ml_rot2rodrigues(Rout, xg);
  xg[3] = tout[0]; xg[4] = tout[1]; xg[5] = tout[2];
  int path = 0;
#pragma unroll 1
  for (int it = 0; it < kMlGnIterations; ++it) {
    MlGn G;
    ml_gn_state(xg, G);
    Q.gn(x, W, S, G);
    double Sm[kMlGnSums], dx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kMlGnSums; ++i) Sm[i] = W.sums[i];
    bool ok = lm_solve<6>(Sm, 0.0, Sm + 21, dx);
    double hi = 0.0, lo = DBL_MAX;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      ok = ok && ml_finite(dx[i]);
      const double a = fabs(dx[i]);
      hi = a > hi ? a : hi;
      lo = a < lo ? a : lo;
    }
    if (!ok) { path += 32; break; }                    // the deviation: x stays
    if (hi > 5.0 || lo > 1.0) { path += 8; break; }    // :744
    const bool below = Q.below(x, W, S, G, dx);
#pragma unroll
    for (int i = 0; i < 6; ++i) xg[i] = xg[i] - dx[i];
    ++path;
    if (below) { path += 16; break; }                  // :748-751
  }
  ml_rodrigues2rot(xg, R);
  t[0] = xg[3]; t[1] = xg[4]; t[2] = xg[5];
  *gn_path = path;
}

// ---- CheckInliers (:262-293) ------------------------------------------------------------------------------------------------------
RGBL_HD bool ml_is_inlier(const MlView& v, const double* R, const double* t, int i) {
  const size_t p = (size_t)v.point[i], ft = (size_t)v.feat[i];
  const float X = v.wpos[3 * p], Y = v.wpos[3 * p + 1], Z = v.wpos[3 * p + 2];
  const float xc = (float)(((R[0] * (double)X + R[1] * (double)Y) + R[2] * (double)Z) + t[0]);
  const float yc = (float)(((R[3] * (double)X + R[4] * (double)Y) + R[5] * (double)Z) + t[1]);
  const float zc = (float)(((R[6] * (double)X + R[7] * (double)Y) + R[8] * (double)Z) + t[2]);
  const float u = fr_quot(v.K[0] * xc, zc) + v.K[2], w = fr_quot(v.K[1] * yc, zc) + v.K[3];   // Pinhole::project
  const float dX = v.xy[2 * ft] - u, dY = v.xy[2 * ft + 1] - w;
  const float error2 = dX * dX + dY * dY;
  return error2 < ml_max_error(v, i);
}
// Rcw / tcw converted to CV_32F and put into a 4 x 4 (:177-183, :338-345), row-major
RGBL_HD void ml_Tcw(const double* R, const double* t, float* T) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T[4 * i] = (float)R[3 * i]; T[4 * i + 1] = (float)R[3 * i + 1]; T[4 * i + 2] = (float)R[3 * i + 2]; T[4 * i + 3] = (float)t[i];
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// ---- the loop of iterate as a scan over the counts (:115-220) ----------------------------------------------------------------------
// Hypothesis k qualifies when c[k] >= min_inliers.  A qualifying c[k] > best makes k the record (mvbBestInliers, mBestTcw).  Then
// Refine (:295-353) runs.  AS COMPILED it does not refine anything: it calls computePose on the record's inliers but never
// copies `result` into mRi / mti (only iterate does, :152-164), so the CheckInliers behind it (:331) evaluates hypothesis k's
// pose once more: mnRefinedInliers = c[k], mvbRefinedInliers = k's flags, and mRefinedTcw (:338-345) is k's pose in float.
// Refine therefore succeeds iff c[k] > min_inliers, and iterate returns hypothesis k - which need not be the record when a
// larger mnBestInliers was carried in from an earlier call.  The recomputed pose has no observable effect and is not computed
// here.  `refines` counts the calls of Refine (the qualifying hypotheses up to the stop).
struct MlScan {
  int32_t found, no_more, n_inliers, iterations, best, record, refines, selected;
};
template <class Counts> RGBL_HD MlScan ml_scan(const Counts& c, int n_hyp, int min_inliers, int best_inliers) {
  MlScan r = {0, 0, 0, n_hyp, best_inliers, -1, 0, -1};
  for (int k = 0; k < n_hyp; ++k) {
    const int ck = c[k];
    if (ck < min_inliers) continue;
    if (ck > r.best) { r.best = ck; r.record = k; }
    ++r.refines;
    if (ck > min_inliers) {
      r.found = 1; r.n_inliers = ck; r.iterations = k + 1; r.selected = k;
      return r;
    }
  }
  r.no_more = 1;
  if (r.best >= min_inliers) { r.found = 1; r.n_inliers = r.best; }   // mBestTcw and mvbBestInliers: the record's, or the carried ones
  return r;
}

}  // namespace rgbl
