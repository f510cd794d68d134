// newpoint_math.h — the per-match block of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:481-710), in ONE place for host
// and device: un-projection and ray parallax (:558-563), the stereo parallax `cos(2*atan2(mb/2, depth))` (:570-572),
// GeometricTools::Triangulate (src/GeometricTools.cc:47-66), KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772), the depth,
// reprojection and scale-consistency tests (:612-691).  Single-camera pinhole key frames (mpCamera2 == nullptr, NLeft == -1).
//
// fp32 in the reference's order, no contraction (-ffp-contract=off), every division and square root correctly rounded (on the
// device through fp64, as frustum_math.h does).  Three-term sums are (a0 b0 + a1 b1) + a2 b2, the order of the Eigen stand-in
// the reference's lines are compiled against in the tests (frustum_math.h says what that does and does not pin).
//
// atan2f / atanf are restated from glibc 2.35 (sysdeps/ieee754/flt-32/e_atan2f.c, s_atanf.c: the fdlibm float forms): under
// `using namespace std` the reference's cos(2*atan2(float, float)) resolves to the float overloads, and neither function is
// correctly rounded.  tests/atanf_sweep.cpp compares both with the live libm bit for bit.
//
// np_triangulate replaces Eigen::JacobiSVD<Matrix4f> (two-sided Jacobi with a QR preconditioner) by a one-sided (Hestenes)
// Jacobi on the columns of the fp32 A, carried out in fp64: NOT the reference's bits - the project's reading, as for every
// Eigen evaluation order - and closer to the exact null vector than any fp32 SVD (DESIGN.md has the figures).  kNpSweeps sweeps
// over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the only data-dependent branch is "skip the rotation when the two
// columns' dot product is exactly 0".
#pragma once
#include <math.h>
#include <stdint.h>

#include "frustum_math.h"
#include "sincos_glibc.h"

namespace rgbl {

constexpr int kNpSweeps = 6;   // chosen once: the Jacobi iteration converges quadratically, 4 x 4 matrices are done after five

// the status byte of a rgbl_new_point (include/rgbl_frontend.h)
enum : uint8_t {
  kNpNone = 0, kNpTriangulated = 1, kNpStereo1 = 2, kNpStereo2 = 3, kNpLowParallax = 4, kNpWZero = 5, kNpNoDepth = 6,
  kNpBehind1 = 7, kNpBehind2 = 8, kNpReproj1 = 9, kNpReproj2 = 10, kNpDistZero = 11, kNpFar = 12, kNpScale = 13
};

RGBL_HD float np_float(uint32_t u) { union { float f; uint32_t u; } c; c.u = u; return c.f; }
RGBL_HD uint32_t np_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
RGBL_HD float np_div(float a, float b) { return fr_quot(a, b); }
RGBL_HD float np_sqrt(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (float)sqrt((double)a);   // rounds to the correctly rounded fp32 root (frustum_math.h)
#else
  return sqrtf(a);
#endif
}

// glibc 2.35 __atanf (s_atanf.c)
RGBL_HD float np_atanf(float x) {
  const float hi[4] = {np_float(0x3eed6338u), np_float(0x3f490fdau), np_float(0x3f7b985eu), np_float(0x3fc90fdau)};
  const float lo[4] = {np_float(0x31ac3769u), np_float(0x33222168u), np_float(0x33140fb4u), np_float(0x33a22168u)};
  const float aT0 = np_float(0x3eaaaaabu), aT1 = np_float(0xbe4ccccdu), aT2 = np_float(0x3e124925u), aT3 = np_float(0xbde38e38u),
              aT4 = np_float(0x3dba2e6eu), aT5 = np_float(0xbd9d8795u), aT6 = np_float(0x3d886b35u), aT7 = np_float(0xbd6ef16bu),
              aT8 = np_float(0x3d4bda59u), aT9 = np_float(0xbd15a221u), aT10 = np_float(0x3c8569d7u);
  const int32_t hx = (int32_t)np_bits(x), ix = hx & 0x7fffffff;
  int id;
  if (ix >= 0x4c000000) {   // |x| >= 2^25
    if (ix > 0x7f800000) return x + x;   // NaN
    return hx > 0 ? hi[3] + lo[3] : -hi[3] - lo[3];
  }
  if (ix < 0x3ee00000) {   // |x| < 0.4375
    if (ix < 0x31000000) return x;   // |x| < 2^-29
    id = -1;
  } else {
    x = fabsf(x);
    if (ix < 0x3f980000) {   // |x| < 1.1875
      if (ix < 0x3f300000) { id = 0; x = np_div(2.0f * x - 1.0f, 2.0f + x); }   // 7/16 <= |x| < 11/16
      else { id = 1; x = np_div(x - 1.0f, x + 1.0f); }                          // 11/16 <= |x| < 19/16
    } else {
      if (ix < 0x401c0000) { id = 2; x = np_div(x - 1.5f, 1.0f + 1.5f * x); }   // |x| < 2.4375
      else { id = 3; x = np_div(-1.0f, x); }
    }
  }
  const float z = x * x, w = z * z;
  const float s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
  const float s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
  if (id < 0) return x - x * (s1 + s2);
  const float r = hi[id] - ((x * (s1 + s2) - lo[id]) - x);
  return hx < 0 ? -r : r;
}

// glibc 2.35 __ieee754_atan2f (e_atan2f.c)
RGBL_HD float np_atan2f(float y, float x) {
  const float tiny = 1.0e-30f, pi_o_4 = np_float(0x3f490fdbu), pi_o_2 = np_float(0x3fc90fdbu), pi = np_float(0x40490fdbu),
              pi_lo = np_float(0xb3bbbd2eu);
  const int32_t hx = (int32_t)np_bits(x), hy = (int32_t)np_bits(y), ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;   // NaN
  if (hx == 0x3f800000) return np_atanf(y);               // x = 1
  const int m = (int)(((uint32_t)hy >> 31) & 1u) | (int)(((uint32_t)hx >> 30) & 2u);   // 2 * sign(x) + sign(y)
  if (iy == 0) {
    if (m < 2) return y;                    // atan(+-0, +anything) = +-0
    return m == 2 ? pi + tiny : -pi - tiny;
  }
  if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (ix == 0x7f800000) {
    if (iy == 0x7f800000) {
      switch (m) {
        case 0: return pi_o_4 + tiny;
        case 1: return -pi_o_4 - tiny;
        case 2: return 3.0f * pi_o_4 + tiny;
        default: return -3.0f * pi_o_4 - tiny;
      }
    }
    switch (m) {
      case 0: return 0.0f;
      case 1: return -0.0f;
      case 2: return pi + tiny;
      default: return -pi - tiny;
    }
  }
  if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int k = (iy - ix) >> 23;
  float z;
  if (k > 60) z = pi_o_2 + 0.5f * pi_lo;        // |y / x| > 2^60
  else if (hx < 0 && k < -60) z = 0.0f;         // |y| / x < -2^60
  else z = np_atanf(fabsf(np_div(y, x)));
  switch (m) {
    case 0: return z;
    case 1: return np_float(np_bits(z) ^ 0x80000000u);
    case 2: return pi - (z - pi_lo);
    default: return (z - pi_lo) - pi;
  }
}

// cos(2 * atan2(mb / 2, depth)) (LocalMapping.cc:570, 572): the float overloads
RGBL_HD float np_cos_parallax_stereo(float mb, float depth) { return glibc_cosf(2.0f * np_atan2f(np_div(mb, 2.0f), depth)); }

// Pinhole::unprojectEig (Pinhole.cpp:61-64); K = fx, fy, cx, cy; z = 1
RGBL_HD void np_unproject(const float K[4], float u, float v, float xn[2]) {
  xn[0] = np_div(u - K[2], K[0]);
  xn[1] = np_div(v - K[3], K[1]);
}
// ray = Rwc * xn with Rwc = Rcw^T (LocalMapping.cc:417, 561); Tcw is 3 x 4 row-major
RGBL_HD void np_ray(const float Tcw[12], const float xn[2], float ray[3]) {
  for (int r = 0; r < 3; ++r) ray[r] = (Tcw[r] * xn[0] + Tcw[4 + r] * xn[1]) + Tcw[8 + r] * 1.0f;
}
// ray1.dot(ray2) / (ray1.norm() * ray2.norm()) (:563)
RGBL_HD float np_cos_parallax_rays(const float a[3], const float b[3]) {
  return np_div(fr_dot(a[0], a[1], a[2], b[0], b[1], b[2]), fr_norm(a[0], a[1], a[2]) * fr_norm(b[0], b[1], b[2]));
}

// What GeometricTools::Triangulate takes from Eigen::JacobiSVD<Matrix4f>(A, ComputeFullV): matrixV().col(3), the right singular
// vector of the smallest singular value of the fp32 A (row-major), by the Jacobi sweeps in fp64 (IEEE division and square root on
// host and device alike, no contraction: the same bits on both), rounded to fp32.
RGBL_HD void np_null_vector(const float A32[16], float h[4]) {
  double A[4][4], V[4][4];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      A[r][c] = (double)A32[4 * r + c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kNpSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < 4; ++r) {
          alpha += A[r][p] * A[r][p];
          beta += A[r][q] * A[r][q];
          gamma += A[r][p] * A[r][q];
        }
        if (gamma == 0.0) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double root = sqrt(1.0 + zeta * zeta);   // inf for a huge zeta: t = 0, no rotation
        const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : -1.0 / (root - zeta);
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 4; ++r) {
          const double ap = A[r][p], aq = A[r][q], vp = V[r][p], vq = V[r][q];
          A[r][p] = c * ap - s * aq;
          A[r][q] = s * ap + c * aq;
          V[r][p] = c * vp - s * vq;
          V[r][q] = s * vp + c * vq;
        }
      }
  int best = 0;
  double least = 0.0;
  for (int c = 0; c < 4; ++c) {
    double n2 = 0.0;
    for (int r = 0; r < 4; ++r) n2 += A[r][c] * A[r][c];
    if (c == 0 || n2 <= least) { least = n2; best = c; }   // ties to the higher index
  }
  // no dynamic indexing of V on the device: select
  for (int r = 0; r < 4; ++r) h[r] = (float)(best == 0 ? V[r][0] : best == 1 ? V[r][1] : best == 2 ? V[r][2] : V[r][3]);
}

// GeometricTools::Triangulate: the rows of A in fp32 as GeometricTools.cc:50-53 write them, the null vector, false when its last
// component is 0, else x3D = head(3) / w in fp32 (the sign of the vector cancels).
RGBL_HD bool np_triangulate(const float xn1[2], const float xn2[2], const float T1[12], const float T2[12], float x3D[3]) {
  float A[16], h[4];
  for (int c = 0; c < 4; ++c) {
    A[c] = xn1[0] * T1[8 + c] - T1[c];
    A[4 + c] = xn1[1] * T1[8 + c] - T1[4 + c];
    A[8 + c] = xn2[0] * T2[8 + c] - T2[c];
    A[12 + c] = xn2[1] * T2[8 + c] - T2[4 + c];
  }
  np_null_vector(A, h);
  if (h[3] == 0.0f) return false;
  x3D[0] = np_div(h[0], h[3]);
  x3D[1] = np_div(h[1], h[3]);
  x3D[2] = np_div(h[2], h[3]);
  return true;
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:755-772): the RAW key point (mvKeys), invfx = 1.0f / fx (Frame.cc), mRwc = Rcw^T,
// mTwc.translation() = the camera centre Ow
RGBL_HD bool np_unproject_stereo(const float K[4], const float Tcw[12], const float Ow[3], float u, float v, float z, float x3D[3]) {
  if (!(z > 0.0f)) return false;
  const float x = (u - K[2]) * z * np_div(1.0f, K[0]);
  const float y = (v - K[3]) * z * np_div(1.0f, K[1]);
  for (int r = 0; r < 3; ++r) x3D[r] = ((Tcw[r] * x + Tcw[4 + r] * y) + Tcw[8 + r] * z) + Ow[r];
  return true;
}

// one key frame's side of a match
struct NpSide {
  float Tcw[12], Ow[3], K[4], mb;
  float u, v, u_raw, v_raw, uright, depth, sigma2, scale;   // mvKeysUn.pt, mvKeys.pt, mvuRight, mvDepth, mvLevelSigma2 / mvScaleFactors[octave]
};
struct NpParams { float mbf1, ratio_factor, th_far_points; int far_points, inertial; };

// reprojection test of one side (:621-647 / :649-672); mbf is ALWAYS the current key frame's (:640, :665)
RGBL_HD bool np_reprojects(const NpSide& S, bool stereo, float mbf, const float x3D[3], float z) {
  const float x = fr_row_times(S.Tcw, x3D[0], x3D[1], x3D[2]) + S.Tcw[3];
  const float y = fr_row_times(S.Tcw + 4, x3D[0], x3D[1], x3D[2]) + S.Tcw[7];
  if (!stereo) {
    const float ex = (np_div(S.K[0] * x, z) + S.K[2]) - S.u, ey = (np_div(S.K[1] * y, z) + S.K[3]) - S.v;   // Pinhole::project
    return !((double)(ex * ex + ey * ey) > 5.991 * (double)S.sigma2);
  }
  const float invz = np_div(1.0f, z);   // 1.0 / z in double, rounded to float: the fp32 quotient
  const float u = S.K[0] * x * invz + S.K[2];
  const float ur = u - mbf * invz;
  const float v = S.K[1] * y * invz + S.K[3];
  const float ex = u - S.u, ey = v - S.v, er = ur - S.uright;
  return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)S.sigma2);
}

// LocalMapping.cc:557-691 for one match; x3D is written for every status but 4, 5 and 6 (zeros there)
RGBL_HD uint8_t np_check(const NpSide& S1, const NpSide& S2, const NpParams& P, float x3D[3]) {
  x3D[0] = x3D[1] = x3D[2] = 0.0f;
  const bool stereo1 = S1.uright >= 0.0f, stereo2 = S2.uright >= 0.0f;
  float xn1[2], xn2[2], ray1[3], ray2[3];
  np_unproject(S1.K, S1.u, S1.v, xn1);
  np_unproject(S2.K, S2.u, S2.v, xn2);
  np_ray(S1.Tcw, xn1, ray1);
  np_ray(S2.Tcw, xn2, ray2);
  const float cos_rays = np_cos_parallax_rays(ray1, ray2);
  float cs1 = cos_rays + 1.0f, cs2 = cs1;
  if (stereo1) cs1 = np_cos_parallax_stereo(S1.mb, S1.depth);
  else if (stereo2) cs2 = np_cos_parallax_stereo(S2.mb, S2.depth);
  const float cos_stereo = cs2 < cs1 ? cs2 : cs1;   // std::min(cs1, cs2)
  uint8_t accepted;
  if (cos_rays < cos_stereo && cos_rays > 0.0f &&
      (stereo1 || stereo2 || ((double)cos_rays < 0.9996 && P.inertial) || ((double)cos_rays < 0.9998 && !P.inertial))) {
    if (!np_triangulate(xn1, xn2, S1.Tcw, S2.Tcw, x3D)) return kNpWZero;
    accepted = kNpTriangulated;
  } else if (stereo1 && cs1 < cs2) {
    if (!np_unproject_stereo(S1.K, S1.Tcw, S1.Ow, S1.u_raw, S1.v_raw, S1.depth, x3D)) return kNpNoDepth;
    accepted = kNpStereo1;
  } else if (stereo2 && cs2 < cs1) {
    if (!np_unproject_stereo(S2.K, S2.Tcw, S2.Ow, S2.u_raw, S2.v_raw, S2.depth, x3D)) return kNpNoDepth;
    accepted = kNpStereo2;
  } else {
    return kNpLowParallax;
  }
  const float z1 = fr_row_times(S1.Tcw + 8, x3D[0], x3D[1], x3D[2]) + S1.Tcw[11];
  if (z1 <= 0.0f) return kNpBehind1;
  const float z2 = fr_row_times(S2.Tcw + 8, x3D[0], x3D[1], x3D[2]) + S2.Tcw[11];
  if (z2 <= 0.0f) return kNpBehind2;
  if (!np_reprojects(S1, stereo1, P.mbf1, x3D, z1)) return kNpReproj1;
  if (!np_reprojects(S2, stereo2, P.mbf1, x3D, z2)) return kNpReproj2;
  const float dist1 = fr_norm(x3D[0] - S1.Ow[0], x3D[1] - S1.Ow[1], x3D[2] - S1.Ow[2]);
  const float dist2 = fr_norm(x3D[0] - S2.Ow[0], x3D[1] - S2.Ow[1], x3D[2] - S2.Ow[2]);
  if (dist1 == 0.0f || dist2 == 0.0f) return kNpDistZero;
  if (P.far_points && (dist1 >= P.th_far_points || dist2 >= P.th_far_points)) return kNpFar;
  const float ratio_dist = np_div(dist2, dist1), ratio_octave = np_div(S1.scale, S2.scale);
  if (ratio_dist * P.ratio_factor < ratio_octave || ratio_dist > ratio_octave * P.ratio_factor) return kNpScale;
  return accepted;
}

}  // namespace rgbl
