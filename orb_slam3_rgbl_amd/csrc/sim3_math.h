// sim3_math.h — Sim3Solver (src/Sim3Solver.cc) for pinhole cameras, in ONE place for host and device: ComputeCentroid and
// ComputeSim3 (:302-412, Horn 1987, steps 1-8, both mbFixScale values, T12 and T21), Project / FromCameraToImage (:461-487) with
// Pinhole::project(const Eigen::Vector3f&) (src/CameraModels/Pinhole.cpp:43-49), CheckInliers (:415-439) and the rule by which
// the loop of iterate (:167-210, :240-288) stops, written as a scan over the inlier counts.
//
// Arithmetic.  fp32 where the reference is fp32: the points, the centroids, M, the float N matrix, the angle-axis vector,
// SO3f::exp, P3, sR, t12, T21, the projections and both squared errors; three-term sums in frustum_math.h's order (left to
// right); every fp32 division and square root is IEEE (through fp64 on the device, as k_frustum does).  fp64 where the
// reference is double: ang = atan2(...), 2 * ang, nom / den and 1.0 / ms12i, each rounded to float where Eigen's scalar
// promotion or the float member rounds it.  The ten N_ij are double VARIABLES, but C++ forms `M(0,0)+M(1,1)+M(2,2)` in float
// before the assignment widens it, and `N << N11, ...` narrows it again: they are float sums here, the same values.
// SO3f::exp is Thirdparty/Sophus/sophus/so3.hpp:583-619 with the small-angle branch (theta^2 < 1e-5f * 1e-5f), the sinf / cosf
// of sincos_glibc.h, and ends in the matrix Eigen's Quaternion::toRotationMatrix makes of the (not re-normalised) quaternion.
// No contraction (-ffp-contract=off).  Host build, emulated kernel and MI355X agree bit for bit, NaN cases included (a NaN
// is compared as a NaN, not by its sign or payload).
//
// What is NOT pinned - the header owns it:
//   - the eigenvector.  The reference runs Eigen::EigenSolver<Matrix4f> (a float general real-Schur solver) and takes the
//     column of eval.maxCoeff().  Here: a cyclic Jacobi on the symmetric 4 x 4 in fp64, kS3Sweeps sweeps of the six rotations
//     (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), no data-dependent exit (a zero off-diagonal entry gives the identity rotation); the
//     first largest diagonal entry wins, as with maxCoeff; the sign is fixed to w >= 0 (Eigen's is whatever the Schur form
//     leaves; q and -q are the same rotation, but atan2 sees the sign of w, so a reference run may take the angle 2 pi - a
//     about the opposite axis - the same matrix up to rounding); the vector is rounded to float;
//   - the double atan2 (s3_atan2 below, so that host and device give the same bits).  `double ang = atan2(...)` reads as a
//     double evaluation and is one here; compiled, the reference's call has two float arguments under a using-directive for
//     std and binds to std::atan2(float, float).  The difference is 4.8e-7 of mBestT12's largest entry at the most on the
//     recorded runs, the same inliers.
//     Against glibc's atan2 (tests/sim3_host_check.cpp, 2 M float-rounded unit vectors and as many scaled ones in all four
//     quadrants): at most 3 ulp apart; a w >= 0 reaches the first quadrant only.  atan2(+-0, -0) gives +-0, not +-pi;
//   - the order of Eigen's small fixed-size products and reductions, as everywhere in this project: written left to right,
//     `(array * array).sum()` column by column, `ms12i * mR12i * O2` as (s R) O2, `-sRinv * mt12i` as (-sRinv) t;
//   - SOPHUS_ENSURE (so3.hpp:614) would abort the reference's process on a NaN quaternion; here the NaN goes on.
//
// Degenerate samples.  Coincident or collinear points can leave a top eigenvector with a zero imaginary part: vec.norm() is 0,
// 2 * ang * vec / 0 is NaN, T12 and T21 are NaN, every error is NaN and NaN is not `<` anything: zero inliers.  A point with
// z == 0 projects to +-inf (or NaN for 0 / 0) and is no inlier.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frustum_math.h"
#include "sincos_glibc.h"

namespace rgbl {

constexpr int kS3Sweeps = 8;   // cyclic Jacobi sweeps: a symmetric 4 x 4 is diagonal to fp64 rounding after 5 or 6

RGBL_HD float s3_sqrtf(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (float)sqrt((double)x);   // IEEE, see fr_norm
#else
  return sqrtf(x);
#endif
}

// ---- atan2 in fp64 -------------------------------------------------------------------------------------------------------
// atan on [0, 1]: x = c + d with c = k / 4 the nearest quarter, atan x = atan c + atan t, t = (x - c) / (1 + x c), |t| <= 1/8,
// and the odd series up to t^25 (the next term is below 2^-82)
RGBL_HD double s3_atan_unit(double x) {
  const int k = (int)(x * 4.0 + 0.5);
  const double c = 0.25 * (double)k;
  const double hi = k == 0 ? 0.0 : k == 1 ? 0x1.f5b75f92c80ddp-3 : k == 2 ? 0x1.dac670561bb4fp-2 : k == 3 ? 0x1.4978fa3269ee1p-1 : 0x1.921fb54442d18p-1;
  const double t = (x - c) / (1.0 + x * c);
  const double z = t * t;
  double q = 1.0 / 25.0;
  q = -1.0 / 23.0 + z * q;
  q = 1.0 / 21.0 + z * q;
  q = -1.0 / 19.0 + z * q;
  q = 1.0 / 17.0 + z * q;
  q = -1.0 / 15.0 + z * q;
  q = 1.0 / 13.0 + z * q;
  q = -1.0 / 11.0 + z * q;
  q = 1.0 / 9.0 + z * q;
  q = -1.0 / 7.0 + z * q;
  q = 1.0 / 5.0 + z * q;
  q = -1.0 / 3.0 + z * q;
  return hi + (t + t * (z * q));
}
RGBL_HD double s3_atan2(double y, double x) {
  if (y != y || x != x) return y + x;
  const double ay = fabs(y), ax = fabs(x);
  double r;
  if (ay == 0.0 && ax == 0.0) return y;
  if (ay > 1.7976931348623157e308 && ax > 1.7976931348623157e308) r = 0x1.921fb54442d18p-1;
  else if (ay <= ax) r = s3_atan_unit(ay / ax);
  else r = 0x1.921fb54442d18p+0 - s3_atan_unit(ax / ay);
  if (x < 0.0) r = 0x1.921fb54442d18p+1 - r;
  return y < 0.0 ? -r : r;
}

// ---- the top eigenvector of a symmetric 4 x 4 ------------------------------------------------------------------------------
// one Jacobi rotation in the (P, Q) plane; P, Q are compile-time so that a and v stay in registers
template <int P, int Q> RGBL_HD void s3_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double t = apq == 0.0 ? 0.0 : tt;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = a[r][P], arq = a[r][Q];
      a[r][P] = c * arp - s * arq;
      a[r][Q] = s * arp + c * arq;
      a[P][r] = a[r][P];
      a[Q][r] = a[r][Q];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = c * vrp - s * vrq;
    v[r][Q] = s * vrp + c * vrq;
  }
}
// n: the ten entries N11 N12 N13 N14 N22 N23 N24 N33 N34 N44 of the float matrix; e: the eigenvector (w x y z), w >= 0
RGBL_HD void s3_top_eigenvector(const float* n, float* e) {
  double a[4][4], v[4][4];
  a[0][0] = n[0]; a[0][1] = n[1]; a[0][2] = n[2]; a[0][3] = n[3];
  a[1][0] = n[1]; a[1][1] = n[4]; a[1][2] = n[5]; a[1][3] = n[6];
  a[2][0] = n[2]; a[2][1] = n[5]; a[2][2] = n[7]; a[2][3] = n[8];
  a[3][0] = n[3]; a[3][1] = n[6]; a[3][2] = n[8]; a[3][3] = n[9];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kS3Sweeps; ++sweep) {
    s3_rotate<0, 1>(a, v);
    s3_rotate<0, 2>(a, v);
    s3_rotate<0, 3>(a, v);
    s3_rotate<1, 2>(a, v);
    s3_rotate<1, 3>(a, v);
    s3_rotate<2, 3>(a, v);
  }
  int idx = 0;
  double top = a[0][0];
  if (a[1][1] > top) { top = a[1][1]; idx = 1; }
  if (a[2][2] > top) { top = a[2][2]; idx = 2; }
  if (a[3][3] > top) { top = a[3][3]; idx = 3; }
  double q[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = idx == 0 ? v[r][0] : idx == 1 ? v[r][1] : idx == 2 ? v[r][2] : v[r][3];
  const bool flip = q[0] < 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) e[r] = (float)(flip ? -q[r] : q[r]);
}

// ---- Sophus::SO3f::exp(omega).matrix() (so3.hpp:583-619, Eigen's toRotationMatrix), row-major -----------------------------
RGBL_HD void s3_so3_exp(const float* om, float* R) {
  const float theta_sq = fr_dot(om[0], om[1], om[2], om[0], om[1], om[2]);
  float imag, real;
  if (!(theta_sq < INFINITY)) {
    imag = real = theta_sq - theta_sq;   // NaN; sinf / cosf of sincos_glibc.h are for finite arguments
  } else if (theta_sq < 1e-5f * 1e-5f) {
    const float theta_po4 = theta_sq * theta_sq;
    imag = 0.5f - (float)(1.0 / 48.0) * theta_sq + (float)(1.0 / 3840.0) * theta_po4;
    real = 1.0f - (float)(1.0 / 8.0) * theta_sq + (float)(1.0 / 384.0) * theta_po4;
  } else {
    const float theta = s3_sqrtf(theta_sq);
    const float half = 0.5f * theta;
    imag = fr_quot(glibc_sinf(half), theta);
    real = glibc_cosf(half);
  }
  const float w = real, x = imag * om[0], y = imag * om[1], z = imag * om[2];
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz;          R[2] = txz + twy;
  R[3] = txy + twz;          R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;          R[7] = tyz + twx;          R[8] = 1.0f - (txx + tyy);
}

// ---- ComputeSim3 (:311-412) ------------------------------------------------------------------------------------------------
struct S3Hyp {
  float R[9];      // mR12i, row-major
  float t[3];      // mt12i
  float s;         // ms12i
  float sR[9];     // T12's rotation block
  float iR[9];     // T21's: sRinv
  float it[3];     // T21's translation
};

// ComputeCentroid (:302-308): P holds the three points as p[3 * k + i] (point k, coordinate i)
RGBL_HD void s3_centroid(const float* P, float* Pr, float* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i) C[i] = fr_quot((P[i] + P[3 + i]) + P[6 + i], 3.0f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) Pr[3 * k + i] = P[3 * k + i] - C[i];
  }
}

RGBL_HD void s3_compute_sim3(const float* P1, const float* P2, int fix_scale, S3Hyp& H) {
  float Pr1[9], Pr2[9], O1[3], O2[3];
  s3_centroid(P1, Pr1, O1);   // step 1
  s3_centroid(P2, Pr2, O2);
  float M[3][3];              // step 2: M = Pr2 * Pr1^T
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = fr_dot(Pr2[i], Pr2[3 + i], Pr2[6 + i], Pr1[j], Pr1[3 + j], Pr1[6 + j]);
  }
  float n[10];                // step 3
  n[0] = M[0][0] + M[1][1] + M[2][2];
  n[1] = M[1][2] - M[2][1];
  n[2] = M[2][0] - M[0][2];
  n[3] = M[0][1] - M[1][0];
  n[4] = M[0][0] - M[1][1] - M[2][2];
  n[5] = M[0][1] + M[1][0];
  n[6] = M[2][0] + M[0][2];
  n[7] = -M[0][0] + M[1][1] - M[2][2];
  n[8] = M[1][2] + M[2][1];
  n[9] = -M[0][0] - M[1][1] + M[2][2];
  float e[4];                 // step 4
  s3_top_eigenvector(n, e);
  const float nrm = fr_norm(e[1], e[2], e[3]);
  const double ang = s3_atan2((double)nrm, (double)e[0]);
  const float two_ang = (float)(2.0 * ang);
  float om[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) om[i] = fr_quot(two_ang * e[1 + i], nrm);
  s3_so3_exp(om, H.R);
  float P3[9];                // step 5: P3 = R * Pr2
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) P3[3 * k + i] = fr_row_times(H.R + 3 * i, Pr2[3 * k], Pr2[3 * k + 1], Pr2[3 * k + 2]);
  }
  if (!fix_scale) {           // step 6
    float nom = 0.0f, den = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      nom += Pr1[k] * P3[k];
      den += P3[k] * P3[k];
    }
    H.s = (float)((double)nom / (double)den);
  } else {
    H.s = 1.0f;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) H.sR[k] = H.s * H.R[k];
#pragma unroll
  for (int i = 0; i < 3; ++i) H.t[i] = O1[i] - fr_row_times(H.sR + 3 * i, O2[0], O2[1], O2[2]);   // step 7
  const float inv = (float)(1.0 / (double)H.s);   // step 8.2
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) H.iR[3 * i + j] = inv * H.R[3 * j + i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float m[3] = {-H.iR[3 * i], -H.iR[3 * i + 1], -H.iR[3 * i + 2]};
    H.it[i] = fr_row_times(m, H.t[0], H.t[1], H.t[2]);
  }
}

// mT12i (:396-400), row-major
RGBL_HD void s3_T12(const S3Hyp& H, float* T) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T[4 * i] = H.sR[3 * i]; T[4 * i + 1] = H.sR[3 * i + 1]; T[4 * i + 2] = H.sR[3 * i + 2]; T[4 * i + 3] = H.t[i];
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// ---- projections and CheckInliers -------------------------------------------------------------------------------------------
// Pinhole::project(const Eigen::Vector3f&) (Pinhole.cpp:43-49); K = fx fy cx cy
RGBL_HD void s3_pinhole(const float* K, const float* X, float* uv) {
  uv[0] = fr_quot(K[0] * X[0], X[2]) + K[2];
  uv[1] = fr_quot(K[1] * X[1], X[2]) + K[3];
}
// Rcw * X + tcw (:107, :110, :471)
RGBL_HD void s3_transform(const float* R, const float* t, const float* X, float* Y) {
#pragma unroll
  for (int i = 0; i < 3; ++i) Y[i] = fr_row_times(R + 3 * i, X[0], X[1], X[2]) + t[i];
}
// one correspondence as CheckInliers sees it: both camera-frame points, both own-image projections, both thresholds
struct S3Point {
  float x1[3], x2[3], p1[2], p2[2], e1, e2;
};
RGBL_HD S3Point s3_point(const float* x1, const float* x2, const float* K1, const float* K2, float e1, float e2) {
  S3Point p;
#pragma unroll
  for (int i = 0; i < 3; ++i) { p.x1[i] = x1[i]; p.x2[i] = x2[i]; }
  s3_pinhole(K1, x1, p.p1);   // FromCameraToImage (:117-118)
  s3_pinhole(K2, x2, p.p2);
  p.e1 = e1; p.e2 = e2;
  return p;
}
RGBL_HD bool s3_is_inlier(const S3Hyp& H, const float* K1, const float* K2, const S3Point& p) {
  float c[3], a[2], b[2];
  s3_transform(H.sR, H.t, p.x2, c);    // Project(mvX3Dc2, vP2im1, mT12i, pCamera1)
  s3_pinhole(K1, c, a);
  s3_transform(H.iR, H.it, p.x1, c);   // Project(mvX3Dc1, vP1im2, mT21i, pCamera2)
  s3_pinhole(K2, c, b);
  const float d10 = p.p1[0] - a[0], d11 = p.p1[1] - a[1];
  const float d20 = b[0] - p.p2[0], d21 = b[1] - p.p2[1];
  const float err1 = d10 * d10 + d11 * d11, err2 = d20 * d20 + d21 * d21;
  return err1 < p.e1 && err2 < p.e2;
}

// ---- the loop of iterate as a scan over the counts (:192-209, :265-287) ------------------------------------------------------
// b = best_inliers on entry; for k = 0 .. n_hyp - 1: c[k] >= b sets b = c[k] and held = k, and if also c[k] > min_inliers the
// scan stops converged.  On a tie the later hypothesis wins.
struct S3Selection {
  int32_t selected, converged, n_inliers, iterations;
};
RGBL_HD S3Selection s3_select(const int32_t* c, int n_hyp, int best_inliers, int min_inliers) {
  S3Selection r = {-1, 0, 0, n_hyp};
  int b = best_inliers;
  for (int k = 0; k < n_hyp; ++k) {
    if (c[k] >= b) {
      b = c[k];
      r.selected = k;
      r.n_inliers = b;
      if (c[k] > min_inliers) {
        r.converged = 1;
        r.iterations = k + 1;
        break;
      }
    }
  }
  return r;
}

}  // namespace rgbl
