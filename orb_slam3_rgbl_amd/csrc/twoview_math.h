// twoview_math.h — TwoViewReconstruction (include/TwoViewReconstruction.h, src/TwoViewReconstruction.cc), the monocular
// initialiser behind Pinhole::ReconstructWithTwoViews (src/CameraModels/Pinhole.cpp:83-92), in ONE place for host and device:
// Normalize (:737-784), ComputeH21 / ComputeF21 (:232-308), the T2inv * Hn * T1, H21i.inverse() and T2t * Fn * T1 of the two
// Find* loops (:131-230), CheckHomography / CheckFundamental (:310-473), DecomposeE (:903-927), the motion hypotheses of
// ReconstructF / ReconstructH (:475-734), CheckRT (:786-901) with GeometricTools::Triangulate (np_triangulate of
// csrc/newpoint_math.h), and the decisions of Reconstruct (:112-128), ReconstructF and ReconstructH.
//
// PINNED - the reference's plain C++, in its own precision and order, no contraction (-ffp-contract=off), every fp32 division
// and square root IEEE (through fp64 on the device, as frustum_math.h does):
//   - Normalize over ALL keys of a frame (not the matched ones): four serial fp32 sums over i = 0 .. n-1, mean = sum / n,
//     sX = 1.0 / meanDevX through double, the normalised point (x - meanX) * sX, T's entries -meanX * sX;
//   - the entries of the 16 x 9 and 8 x 9 matrices A as fp32 products;
//   - CheckHomography / CheckFundamental: the fp32 three-term sums left to right, `1.0 / (...)` through double, invSigmaSquare
//     = 1.0 / (sigma * sigma) through double, th = 5.991f / 3.841f, `chiSquare > th` (a NaN chiSquare is NOT > th: it is added,
//     the score turns NaN and the match stays an inlier), and the SERIAL fp32 accumulation of score over i = 0 .. N-1, two
//     additions per match.  A term the reference skips is added here as +0.0f: the score starts at +0 and every kept term is
//     >= +0 or NaN, so the bits are the same.  On the device the terms of 64 matches are computed across the wave and then
//     added in the reference's order (tv_add_chunk): no tree;
//   - `currentScore > score` with score = 0 at the start: the first strictly greater score wins, a NaN score never does;
//   - SH + SF == 0.f, RH = SH / (SH + SF), RH > 0.50;
//   - ReconstructH: d1 / d2 < 1.00001 || d2 / d3 < 1.00001 (fp32 quotient, double comparison), aux1, aux3, aux_stheta, ctheta,
//     aux_sphi, cphi in fp32 with std::sqrt(float), tp *= d1 -+ d3;
//   - CheckRT: th2 = 4.0 * mSigma2 through double, the isfinite test, `p3dC1(2) <= 0 && cosParallax < 0.99998` (double
//     comparison), invZ = 1.0 / z through double, fx * x * invZ + cx, the squared errors, `> th2` (NaN passes), nGood,
//     vbGood / vP3D by the index of FRAME 1 with non-inliers left at their defaults, vCosParallax[min(50, size - 1)] after the
//     sort, `* 180 / CV_PI` (float product, double quotient, rounded to float), parallax = 0 for nGood == 0;
//   - nMinGood = max(int(0.9 * N), 50), nGood_i > 0.7 * maxGood, maxGood < nMinGood || nsimilar > 1, the else-if chain of
//     ReconstructF (only the FIRST of equal nGood is looked at, and false if that one lacks parallax), parallax > minParallax
//     there and bestParallax >= minParallax in ReconstructH, secondBestGood < 0.75 * bestGood, bestGood > 50, bestGood > 0.9 * N.
//
// NOT pinned - what Eigen computes is the header's own, in fp64 with fixed sweeps and no data-dependent exit, rounded to float
// where the reference holds a float (Eigen's JacobiSVD bits and sign conventions, its product order, libm's acos are not
// reproduced):
//   - the right singular vector of the smallest singular value of A: the eigenvector of the smallest eigenvalue of A^T A (the
//     products of two fp32 entries are exact in fp64, each of the 45 sums runs over the rows in ascending order), by
//     ml_smallest_eigenvector of csrc/mlpnp_math.h (round-robin Jacobi, kMlSweeps sweeps, in the wave's LDS work space); the
//     sign is fixed so that the entry of largest magnitude (the first of equals) is positive.  A sign flip changes no score
//     bit - every quotient of both Check* functions is sign-invariant - but host build, emulator and GPU must agree;
//   - the 3 x 3 SVDs (tv_svd3): V and the order from ml_eig3 on M^T M (descending), w_i = |M v_i|, u_i = M v_i / w_i for the two
//     largest, u_3 = +-(u_1 x u_2) with the sign det M and det V give.  ComputeF21's rank-2 projection U diag(w1, w2, 0) V^T
//     is formed as written, U * diag(w1, w2, 0) * V^T left to right with w rounded to float (the reference holds it in a Vector3f);
//   - 3 x 3 inverses (adjugate over determinant, one division per entry), determinants and products (left to right) in fp64;
//     norms and dot products of Eigen vectors in fp64, rounded to float;
//   - acos: `acos(vCosParallax[idx])` (:895) has a float argument under a using-directive for std, so overload resolution takes
//     std::acos(float): a float result.  The header follows that overload's TYPE: tv_acosf evaluates ml_acos in fp64 and rounds
//     to float before `* 180`.  libm's acosf bits are not reproduced (tests/twoview_host_check.cpp has the distance);
//   - Sophus::SE3f(R, t) stores a quaternion; T21 is handed out as the R and t given to that constructor.
//
// QUIRKS kept as compiled:
//   - FindFundamental sizes its vectors by vbMatchesInliers.size() of the EMPTY argument (:185); only CheckFundamental's resize
//     makes them N.  So when no F hypothesis scores > 0 the F mask stays EMPTY and F21 unset (H: an all-false mask, H21 unset).
//     Reconstruct never reads the side whose score is 0: SF == 0 < SH gives RH = 1 > 0.5, the H path; SH == 0 < SF gives
//     RH = 0, the F path; both 0 is the first exit.  tv_choose_model below is that rule; best_h / best_f are -1 for such a side;
//   - ReconstructH never assigns vP3D: bestP3D is dropped at :725-731 (p3d_assigned = 0 in the C ABI);
//   - ReconstructH tests bestParallax >= minParallax, ReconstructF parallax > minParallax;
//   - CheckRT takes vCosParallax[min(50, size - 1)].
// DEVIATIONS where the reference is undefined: Triangulate returning false (w == 0) leaves p3dC1 uninitialised and CheckRT
// reads it; here such a match is skipped like a non-finite point.  std::sort over a NaN cosParallax is undefined; here the
// NaN values are left out of the order, and an index past the values that remain gives a NaN parallax.
#pragma once
#include "mlpnp_math.h"
#include "newpoint_math.h"

namespace rgbl {

constexpr int kTvMaxMotions = 8;

// exits of Reconstruct / ReconstructF / ReconstructH (rgbl_two_view_output::exit_code)
enum : int32_t {
  kTvFound = 0, kTvNoScore = 1 /* :113 */, kTvHRatio = 2 /* :597-600 */, kTvHRule = 3 /* :725-733 */,
  kTvFFewOrSimilar = 4 /* :520-523 */, kTvFParallax = 5 /* :568 */
};

// one problem as the arithmetic reads it (host arrays or device arrays)
struct TvView {
  const float *xy1, *xy2;        // mvKeys1 / mvKeys2 .pt
  const int32_t *m1, *m2;        // mvMatches12[i].first / .second
  int N, n1, n2;
  float K[4], sigma;
  float T1[4], T2[4];            // Normalize: sX, sY, meanX, meanY
};

struct TvHostX {
  int lane = 0, lanes = 1;
  void sync() {}
  bool all(bool p) { return p; }
};
// the work space of one wave: LDS on the device
struct TvWork {
  MlWork ml;
  double rows[16][9];
  float terms[128];
};

// ---- Normalize (:737-784) ---------------------------------------------------------------------------------------------------------
// buf: 2 x 64 floats of the lanes' work space.  The lanes stage 64 keys; EVERY lane then adds both serial chains in index
// order, so the sums are the reference's and are the same in every lane.
template <class X> RGBL_HD void tv_normalize(X& x, float (*buf)[64], const float* xy, int n, float* T) {
  float mean[2] = {0.0f, 0.0f}, sc[2] = {0.0f, 0.0f};
  for (int pass = 0; pass < 2; ++pass) {
    float ax = 0.0f, ay = 0.0f;
    for (int base = 0; base < n; base += 64) {
      x.sync();
      for (int j = x.lane; j < 64; j += x.lanes) {
        const int i = base + j;
        float vx = 0.0f, vy = 0.0f;
        if (i < n) { vx = xy[2 * (size_t)i]; vy = xy[2 * (size_t)i + 1]; }
        buf[0][j] = pass ? fabsf(vx - mean[0]) : vx;
        buf[1][j] = pass ? fabsf(vy - mean[1]) : vy;
      }
      x.sync();
      const int cnt = n - base < 64 ? n - base : 64;
      for (int j = 0; j < cnt; ++j) { ax = ax + buf[0][j]; ay = ay + buf[1][j]; }
    }
    const float qx = fr_quot(ax, (float)n), qy = fr_quot(ay, (float)n);
    if (pass == 0) { mean[0] = qx; mean[1] = qy; }
    else { sc[0] = (float)(1.0 / (double)qx); sc[1] = (float)(1.0 / (double)qy); }
  }
  T[0] = sc[0]; T[1] = sc[1]; T[2] = mean[0]; T[3] = mean[1];
}
// T as the 3 x 3 the reference fills (:778-783), row-major, in double
RGBL_HD void tv_T3(const float* T, double* M) {
  M[0] = (double)T[0]; M[1] = 0.0; M[2] = (double)(-T[2] * T[0]);
  M[3] = 0.0; M[4] = (double)T[1]; M[5] = (double)(-T[3] * T[1]);
  M[6] = 0.0; M[7] = 0.0; M[8] = 1.0;
}

// ---- 3 x 3 algebra in fp64 (row-major) ---------------------------------------------------------------------------------------------
RGBL_HD void tv_mul3(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
  }
}
RGBL_HD void tv_transpose3(const double* A, double* B) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) B[3 * i + j] = A[3 * j + i];
  }
}
RGBL_HD void tv_inv3(const double* A, double* B) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
  B[0] = c00 / det; B[1] = (A[2] * A[7] - A[1] * A[8]) / det; B[2] = (A[1] * A[5] - A[2] * A[4]) / det;
  B[3] = c01 / det; B[4] = (A[0] * A[8] - A[2] * A[6]) / det; B[5] = (A[2] * A[3] - A[0] * A[5]) / det;
  B[6] = c02 / det; B[7] = (A[1] * A[6] - A[0] * A[7]) / det; B[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}
RGBL_HD void tv_round3(const double* A, float* B) {
#pragma unroll
  for (int i = 0; i < 9; ++i) B[i] = (float)A[i];
}
RGBL_HD void tv_widen3(const float* A, double* B) {
#pragma unroll
  for (int i = 0; i < 9; ++i) B[i] = (double)A[i];
}
// the SVD of a 3 x 3: U, V row-major with the vectors in their columns, w descending
RGBL_HD void tv_svd3(const double* M, double* U, double* w, double* V) {
  double b[6];   // M^T M
  b[0] = M[0] * M[0] + M[3] * M[3] + M[6] * M[6];
  b[1] = M[0] * M[1] + M[3] * M[4] + M[6] * M[7];
  b[2] = M[0] * M[2] + M[3] * M[5] + M[6] * M[8];
  b[3] = M[1] * M[1] + M[4] * M[4] + M[7] * M[7];
  b[4] = M[1] * M[2] + M[4] * M[5] + M[7] * M[8];
  b[5] = M[2] * M[2] + M[5] * M[5] + M[8] * M[8];
  double e[3], v[3][3], u[3][3];
  ml_eig3(b, true, e, v);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double vc[3] = {v[0][c], v[1][c], v[2][c]};
    double m[3];
    ml_matvec(M, vc, m);
    w[c] = ml_norm(m);
    u[0][c] = m[0] / w[c]; u[1][c] = m[1] / w[c]; u[2][c] = m[2] / w[c];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) V[3 * i + j] = v[i][j];
  }
  const double sg = (ml_det3(V) < 0.0 ? -1.0 : 1.0) * (ml_det3(M) < 0.0 ? -1.0 : 1.0);
  const double u0[3] = {u[0][0], u[1][0], u[2][0]}, u1[3] = {u[0][1], u[1][1], u[2][1]};
  double u2[3];
  ml_cross(u0, u1, u2);
#pragma unroll
  for (int i = 0; i < 3; ++i) { U[3 * i] = u[i][0]; U[3 * i + 1] = u[i][1]; U[3 * i + 2] = sg * u2[i]; }
}
// acos of a float as std::acos(float) types it: a float
RGBL_HD float tv_acosf(float x) { return (float)ml_acos((double)x); }
// acos(c) * 180 / CV_PI assigned to a float (:895)
RGBL_HD float tv_parallax_deg(float c) { return (float)((double)(tv_acosf(c) * 180.0f) / 3.1415926535897932384626433832795); }

// ---- the minimal sets: ComputeH21 / ComputeF21 (:232-308) ----------------------------------------------------------------------------
RGBL_HD void tv_normalized(const TvView& v, int idx, float* p1, float* p2) {
  const size_t a = (size_t)v.m1[idx], b = (size_t)v.m2[idx];
  p1[0] = (v.xy1[2 * a] - v.T1[2]) * v.T1[0]; p1[1] = (v.xy1[2 * a + 1] - v.T1[3]) * v.T1[1];
  p2[0] = (v.xy2[2 * b] - v.T2[2]) * v.T2[0]; p2[1] = (v.xy2[2 * b + 1] - v.T2[3]) * v.T2[1];
}
// row r of A: 16 rows of the homography system, 8 of the fundamental one
RGBL_HD void tv_row(const TvView& v, const int32_t* set, bool fundamental, int r, double* row) {
  float p1[2], p2[2];
  tv_normalized(v, set[fundamental ? r : r >> 1], p1, p2);
  const float u1 = p1[0], v1 = p1[1], u2 = p2[0], v2 = p2[1];
  float a[9];
  if (fundamental) {
    a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.0f;
  } else if ((r & 1) == 0) {
    a[0] = 0.0f; a[1] = 0.0f; a[2] = 0.0f; a[3] = -u1; a[4] = -v1; a[5] = -1.0f; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2;
  } else {
    a[0] = u1; a[1] = v1; a[2] = 1.0f; a[3] = 0.0f; a[4] = 0.0f; a[5] = 0.0f; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2;
  }
#pragma unroll
  for (int c = 0; c < 9; ++c) row[c] = (double)a[c];
}
// svd.matrixV().col(8) of the A whose rows lie in W.rows[0 .. nrows), rounded to float
template <class X> RGBL_HD void tv_null_vector_rows(X& x, TvWork& W, int nrows, float* h);
// ... of the set's A
template <class X> RGBL_HD void tv_null_vector(X& x, TvWork& W, const TvView& v, const int32_t* set, bool fundamental, float* h) {
  const int nrows = fundamental ? 8 : 16;
  x.sync();
  for (int r = x.lane; r < nrows; r += x.lanes) {
    double row[9];
    tv_row(v, set, fundamental, r, row);
#pragma unroll
    for (int c = 0; c < 9; ++c) W.rows[r][c] = row[c];
  }
  tv_null_vector_rows(x, W, nrows, h);
}
template <class X> RGBL_HD void tv_null_vector_rows(X& x, TvWork& W, int nrows, float* h) {
  x.sync();
  for (int e = x.lane; e < 45; e += x.lanes) {
    int i, j;
    ml_tri(e, 9, &i, &j);
    double s = 0.0;
    for (int r = 0; r < nrows; ++r) s = s + W.rows[r][i] * W.rows[r][j];
    W.ml.sums[e] = s;
  }
  x.sync();
  const int col = ml_smallest_eigenvector(x, W.ml, 9);
  double n[9], top = 0.0, sg = 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    n[i] = W.ml.V[i][col];
    if (fabs(n[i]) > top) { top = fabs(n[i]); sg = n[i] < 0.0 ? -1.0 : 1.0; }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = (float)(sg * n[i]);
  x.sync();
}
// H21i = T2inv * Hn * T1 and H12i = H21i.inverse() (:141, :166-168)
RGBL_HD void tv_h_models(const float* hn, const TvView& v, float* H21, float* H12) {
  double T1[9], T2[9], Ti[9], Hn[9], A[9], B[9];
  tv_T3(v.T1, T1);
  tv_T3(v.T2, T2);
  tv_inv3(T2, A);
  float T2inv[9];
  tv_round3(A, T2inv);          // Eigen::Matrix3f T2inv
  tv_widen3(T2inv, Ti);
  tv_widen3(hn, Hn);
  tv_mul3(Ti, Hn, A);
  tv_mul3(A, T1, B);
  tv_round3(B, H21);
  tv_widen3(H21, A);
  tv_inv3(A, B);
  tv_round3(B, H12);
}
// Fn = U diag(w1, w2, 0) V^T of Fpre (:300-307), F21i = T2t * Fn * T1 (:192, :219)
RGBL_HD void tv_f_model(const float* fpre, const TvView& v, float* F21) {
  double M[9], U[9], w[3], V[9], P[9];
  tv_widen3(fpre, M);
  tv_svd3(M, U, w, V);
  // Eigen::Vector3f w = singularValues(); w(2) = 0; U * DiagonalMatrix(w) * V^T, left to right
  const double wf[3] = {(double)(float)w[0], (double)(float)w[1], 0.0};
  double UD[9], Vt[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) UD[3 * i + k] = U[3 * i + k] * wf[k];
  }
  tv_transpose3(V, Vt);
  tv_mul3(UD, Vt, P);
  float Fn[9];
  tv_round3(P, Fn);             // what ComputeF21 returns
  double T1[9], T2[9], T2t[9], F[9], A[9], B[9];
  tv_T3(v.T1, T1);
  tv_T3(v.T2, T2);
  tv_transpose3(T2, T2t);
  tv_widen3(Fn, F);
  tv_mul3(T2t, F, A);
  tv_mul3(A, T1, B);
  tv_round3(B, F21);
}

// ---- CheckHomography / CheckFundamental (:310-473) for one match ------------------------------------------------------------------------
RGBL_HD float tv_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
// t[0], t[1]: what the two tests add to the score (+0.0f where the reference adds nothing); returns bIn
RGBL_HD bool tv_check_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare, float* t) {
  const float th = 5.991f;
  bool bIn = true;
  const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
  const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) { bIn = false; t[0] = 0.0f; }
  else t[0] = th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
  const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) { bIn = false; t[1] = 0.0f; }
  else t[1] = th - chiSquare2;
  return bIn;
}
RGBL_HD bool tv_check_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float* t) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = fr_quot(num2 * num2, a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > th) { bIn = false; t[0] = 0.0f; }
  else t[0] = thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = fr_quot(num1 * num1, a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > th) { bIn = false; t[1] = 0.0f; }
  else t[1] = thScore - chiSquare2;
  return bIn;
}
// model: 0 = homography (M = H21, M2 = H12), 1 = fundamental
RGBL_HD bool tv_check(int model, const float* M, const float* M2, const TvView& v, int i, float invSigmaSquare, float* t) {
  const size_t a = (size_t)v.m1[i], b = (size_t)v.m2[i];
  const float u1 = v.xy1[2 * a], v1 = v.xy1[2 * a + 1], u2 = v.xy2[2 * b], v2 = v.xy2[2 * b + 1];
  return model == 0 ? tv_check_h(M, M2, u1, v1, u2, v2, invSigmaSquare, t) : tv_check_f(M, u1, v1, u2, v2, invSigmaSquare, t);
}
// the terms of up to 64 matches, two per match in index order, added to the score as the reference's loop adds them
RGBL_HD float tv_add_chunk(float score, const float* terms, int count) {
  for (int j = 0; j < count; ++j) score = score + terms[j];
  return score;
}
// the models of one (hypothesis, model): M = H21i / F21i, M2 = H12i (homography only)
template <class X> RGBL_HD void tv_model(X& x, TvWork& W, const TvView& v, const int32_t* set, int model, float* M, float* M2) {
  float h[9];
  tv_null_vector(x, W, v, set, model == 1, h);
  if (model == 0) tv_h_models(h, v, M, M2);
  else {
    tv_f_model(h, v, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) M2[i] = 0.0f;
  }
}

// ---- the winners (:155-178, :206-229) and Reconstruct's choice (:112-128) -------------------------------------------------------------
// scores: n_hyp x 2 (homography, fundamental).  The first strictly greater score; -1 when none is > 0.
RGBL_HD int tv_first_max(const float* scores, int n_hyp, int model, float* best) {
  float score = 0.0f;
  int at = -1;
  for (int it = 0; it < n_hyp; ++it) {
    const float c = scores[2 * (size_t)it + model];
    if (c > score) { score = c; at = it; }
  }
  *best = score;
  return at;
}
// 0: ReconstructH, 1: ReconstructF, -1: the exit of :113
RGBL_HD int tv_choose_model(float SH, float SF) {
  if (SH + SF == 0.0f) return -1;
  const float RH = fr_quot(SH, SH + SF);
  return (double)RH > 0.50 ? 0 : 1;
}

// ---- the motion hypotheses ------------------------------------------------------------------------------------------------------------------
struct TvMotions {
  int32_t n;                     // 4 (ReconstructF), 8 (ReconstructH), 0 (the d1 / d2, d2 / d3 exit)
  float R[kTvMaxMotions][9], t[kTvMaxMotions][3];
};
RGBL_HD void tv_K3(const float* K, double* M) {
  M[0] = (double)K[0]; M[1] = 0.0; M[2] = (double)K[2];
  M[3] = 0.0; M[4] = (double)K[1]; M[5] = (double)K[3];
  M[6] = 0.0; M[7] = 0.0; M[8] = 1.0;
}
RGBL_HD void tv_unit3(const float* a, float* b) {   // t / t.norm()
  const double x = (double)a[0], y = (double)a[1], z = (double)a[2];
  const double n = (double)(float)sqrt((x * x + y * y) + z * z);
  b[0] = (float)(x / n); b[1] = (float)(y / n); b[2] = (float)(z / n);
}
// ReconstructF :484-503 with DecomposeE: (R1, t), (R2, t), (R1, -t), (R2, -t)
RGBL_HD void tv_motions_f(const float* F21, const float* K, TvMotions& m) {
  double Kd[9], Kt[9], F[9], A[9], B[9];
  tv_K3(K, Kd);
  tv_transpose3(Kd, Kt);
  tv_widen3(F21, F);
  tv_mul3(Kt, F, A);
  tv_mul3(A, Kd, B);
  float E21[9];
  tv_round3(B, E21);
  double E[9], U[9], w[3], V[9];
  tv_widen3(E21, E);
  tv_svd3(E, U, w, V);
  float Uf[9], Vtf[9];
  double Vt[9];
  tv_round3(U, Uf);
  tv_transpose3(V, Vt);
  tv_round3(Vt, Vtf);
  const float tc[3] = {Uf[2], Uf[5], Uf[8]};
  float t[3];
  tv_unit3(tc, t);
  double Ud[9], Vd[9];
  tv_widen3(Uf, Ud);
  tv_widen3(Vtf, Vd);
  const double Wm[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  double Wt[9], R1[9], R2[9];
  tv_transpose3(Wm, Wt);
  tv_mul3(Ud, Wm, A);
  tv_mul3(A, Vd, R1);
  tv_mul3(Ud, Wt, A);
  tv_mul3(A, Vd, R2);
  float R1f[9], R2f[9];
  tv_round3(R1, R1f);
  tv_round3(R2, R2f);
  tv_widen3(R1f, R1);
  tv_widen3(R2f, R2);
  const bool n1 = ml_det3(R1) < 0.0, n2 = ml_det3(R2) < 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) { R1f[i] = n1 ? -R1f[i] : R1f[i]; R2f[i] = n2 ? -R2f[i] : R2f[i]; }
  m.n = 4;
#pragma unroll
  for (int k = 0; k < kTvMaxMotions; ++k) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m.R[k][i] = k < 4 ? ((k & 1) ? R2f[i] : R1f[i]) : 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) m.t[k][i] = k < 4 ? (k < 2 ? t[i] : -t[i]) : 0.0f;
  }
}
// ReconstructH :582-690 (Faugeras' eight); false: the exit of :597-600
RGBL_HD bool tv_motions_h(const float* H21, const float* K, TvMotions& m) {
  double Kd[9], Ki[9], H[9], A[9], B[9];
  tv_K3(K, Kd);
  tv_inv3(Kd, Ki);
  float invK[9], Af[9];
  tv_round3(Ki, invK);
  tv_widen3(invK, Ki);
  tv_widen3(H21, H);
  tv_mul3(Ki, H, A);
  tv_mul3(A, Kd, B);
  tv_round3(B, Af);
  double Ad[9], U[9], wd[3], V[9], Vt[9];
  tv_widen3(Af, Ad);
  tv_svd3(Ad, U, wd, V);
  float Uf[9], Vf[9];
  tv_round3(U, Uf);
  tv_round3(V, Vf);
  tv_widen3(Uf, U);
  tv_widen3(Vf, V);
  tv_transpose3(V, Vt);
  const float s = (float)(ml_det3(U) * ml_det3(Vt));
  const float d1 = (float)wd[0], d2 = (float)wd[1], d3 = (float)wd[2];
  m.n = 0;
#pragma unroll
  for (int k = 0; k < kTvMaxMotions; ++k) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m.R[k][i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) m.t[k][i] = 0.0f;
  }
  if ((double)fr_quot(d1, d2) < 1.00001 || (double)fr_quot(d2, d3) < 1.00001) return false;
  const float aux1 = np_sqrt(fr_quot(d1 * d1 - d2 * d2, d1 * d1 - d3 * d3));
  const float aux3 = np_sqrt(fr_quot(d2 * d2 - d3 * d3, d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = fr_quot(np_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 + d3) * d2);
  const float ctheta = fr_quot(d2 * d2 + d1 * d3, (d1 + d3) * d2);
  const float aux_sphi = fr_quot(np_sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 - d3) * d2);
  const float cphi = fr_quot(d1 * d3 - d2 * d2, (d1 - d3) * d2);
  double sU[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) sU[i] = (double)s * U[i];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = k & 3;
    const bool second = k >= 4;
    const float st = (i == 0 || i == 3) ? (second ? aux_sphi : aux_stheta) : (second ? -aux_sphi : -aux_stheta);
    double Rp[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!second) { Rp[0] = (double)ctheta; Rp[2] = (double)-st; Rp[4] = 1.0; Rp[6] = (double)st; Rp[8] = (double)ctheta; }
    else { Rp[0] = (double)cphi; Rp[2] = (double)st; Rp[4] = -1.0; Rp[6] = (double)st; Rp[8] = (double)-cphi; }
    tv_mul3(sU, Rp, A);
    tv_mul3(A, Vt, B);
    tv_round3(B, m.R[k]);
    const float scale = second ? d1 + d3 : d1 - d3;
    const float tp[3] = {x1[i] * scale, 0.0f * scale, (second ? x3[i] : -x3[i]) * scale};
    const double tpd[3] = {(double)tp[0], (double)tp[1], (double)tp[2]};
    double td[3];
    ml_matvec(U, tpd, td);
    const float tf[3] = {(float)td[0], (float)td[1], (float)td[2]};
    tv_unit3(tf, m.t[k]);
  }
  m.n = 8;
  return true;
}

// ---- CheckRT (:786-901) ------------------------------------------------------------------------------------------------------------------
struct TvCam {
  float K[4], R[9], t[3], P1[12], P2[12], O2[3], th2;
};
RGBL_HD void tv_cam(const float* K, const float* R, const float* t, float sigma, TvCam& c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) c.K[i] = K[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) c.R[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.t[i] = t[i];
  const float P1[12] = {K[0], 0.0f, K[2], 0.0f, 0.0f, K[1], K[3], 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 12; ++i) c.P1[i] = P1[i];
  double Kd[9];
  tv_K3(K, Kd);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double a0 = j < 3 ? (double)R[j] : (double)t[0], a1 = j < 3 ? (double)R[3 + j] : (double)t[1], a2 = j < 3 ? (double)R[6 + j] : (double)t[2];
      c.P2[4 * i + j] = (float)((Kd[3 * i] * a0 + Kd[3 * i + 1] * a1) + Kd[3 * i + 2] * a2);
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) c.O2[i] = (float)(((-(double)R[i]) * (double)t[0] + (-(double)R[3 + i]) * (double)t[1]) + (-(double)R[6 + i]) * (double)t[2]);
  const float sigma2 = sigma * sigma;
  c.th2 = (float)(4.0 * (double)sigma2);
}
RGBL_HD bool tv_finitef(float x) { return x >= -FLT_MAX && x <= FLT_MAX; }
// one inlier match: 0 = not counted, 1 = counted in nGood (p and *cosv are its vP3D entry and its vCosParallax entry),
// 2 = counted and vbGood
RGBL_HD int tv_rt_point(const TvCam& c, float u1, float v1, float u2, float v2, float* p, float* cosv) {
  const float x1[2] = {u1, v1}, x2[2] = {u2, v2};
  float X[3] = {0.0f, 0.0f, 0.0f};
  if (!np_triangulate(x1, x2, c.P1, c.P2, X)) return 0;
  if (!tv_finitef(X[0]) || !tv_finitef(X[1]) || !tv_finitef(X[2])) return 0;
  const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]};
  const double n2[3] = {(double)(X[0] - c.O2[0]), (double)(X[1] - c.O2[1]), (double)(X[2] - c.O2[2])};
  const float dist1 = (float)ml_norm(Xd), dist2 = (float)ml_norm(n2);
  const float cosParallax = fr_quot((float)ml_dot(Xd, n2), dist1 * dist2);
  const bool low = (double)cosParallax < 0.99998;
  if (X[2] <= 0.0f && low) return 0;
  float X2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    X2[i] = (float)((((double)c.R[3 * i] * Xd[0] + (double)c.R[3 * i + 1] * Xd[1]) + (double)c.R[3 * i + 2] * Xd[2]) + (double)c.t[i]);
  if (X2[2] <= 0.0f && low) return 0;
  const float invZ1 = (float)(1.0 / (double)X[2]);
  const float im1x = c.K[0] * X[0] * invZ1 + c.K[2], im1y = c.K[1] * X[1] * invZ1 + c.K[3];
  const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
  if (squareError1 > c.th2) return 0;
  const float invZ2 = (float)(1.0 / (double)X2[2]);
  const float im2x = c.K[0] * X2[0] * invZ2 + c.K[2], im2y = c.K[1] * X2[1] * invZ2 + c.K[3];
  const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
  if (squareError2 > c.th2) return 0;
  p[0] = X[0]; p[1] = X[1]; p[2] = X[2];
  *cosv = cosParallax;
  return low ? 2 : 1;
}

// ---- the decisions of ReconstructF (:505-568) and ReconstructH (:693-733) ------------------------------------------------------------------
struct TvDecision {
  int32_t found, exit_code, best, aux;   // best: the motion hypothesis looked at (-1: none); aux: nsimilar (F) / secondBestGood (H)
};
RGBL_HD TvDecision tv_decide_f(const int32_t* nGood, const float* parallax, int N) {
  const float minParallax = 1.0f;
  const int minTriangulated = 50;
  int maxGood = nGood[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) maxGood = nGood[i] > maxGood ? nGood[i] : maxGood;
  const int n9 = (int)(0.9 * (double)N);
  const int nMinGood = n9 > minTriangulated ? n9 : minTriangulated;
  int nsimilar = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) nsimilar += (double)nGood[i] > 0.7 * (double)maxGood ? 1 : 0;
  TvDecision d = {0, kTvFFewOrSimilar, -1, nsimilar};
  if (maxGood < nMinGood || nsimilar > 1) return d;
  const int first = maxGood == nGood[0] ? 0 : maxGood == nGood[1] ? 1 : maxGood == nGood[2] ? 2 : 3;
  const float par = first == 0 ? parallax[0] : first == 1 ? parallax[1] : first == 2 ? parallax[2] : parallax[3];
  d.best = first;
  d.exit_code = kTvFParallax;
  if (par > minParallax) { d.found = 1; d.exit_code = kTvFound; }
  return d;
}
RGBL_HD TvDecision tv_decide_h(const int32_t* nGood, const float* parallax, int N) {
  const float minParallax = 1.0f;
  const int minTriangulated = 50;
  int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
  float bestParallax = -1.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (nGood[i] > bestGood) { secondBestGood = bestGood; bestGood = nGood[i]; bestSolutionIdx = i; bestParallax = parallax[i]; }
    else if (nGood[i] > secondBestGood) secondBestGood = nGood[i];
  }
  TvDecision d = {0, kTvHRule, bestSolutionIdx, secondBestGood};
  if ((double)secondBestGood < 0.75 * (double)bestGood && bestParallax >= minParallax && bestGood > minTriangulated && (double)bestGood > 0.9 * (double)N) {
    d.found = 1; d.exit_code = kTvFound;
  }
  return d;
}

}  // namespace rgbl
