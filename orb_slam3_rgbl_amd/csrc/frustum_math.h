// frustum_math.h — the three fixed-size Eigen reductions of Frame::isInFrustum (src/Frame.cc:602-664), in ONE place, and the
// quotient MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:426-494) needs besides them.
//
// The order is the one the Eigen stand-in oracle/cvcompat/sophus/sim3.hpp defines (the stand-in is what the reference's own
// lines are compiled against in the tests): products summed left to right.  Real Eigen's fixed-size redux may group a
// three-term sum as p0 + (p1 + p2); nothing in this repository can decide that ("parity unpinned") - if it does,
// these three functions are what changes.  fp32, no contraction (-ffp-contract=off), host and device.
#pragma once
#include <math.h>

#ifndef RGBL_HD
#if defined(__HIPCC__)
#define RGBL_HD __host__ __device__ inline
#else
#define RGBL_HD inline
#endif
#endif

namespace rgbl {

// Eigen::Matrix3f * Eigen::Vector3f (`mRcw * P`, Frame.cc:613), one row: (m0 p0 + m1 p1) + m2 p2
RGBL_HD float fr_row_times(const float* m, float p0, float p1, float p2) { return m[0] * p0 + m[1] * p1 + m[2] * p2; }

// MatrixBase::dot (`PO.dot(Pn)`, Frame.cc:644) and squaredNorm: sequential
RGBL_HD float fr_dot(float a0, float a1, float a2, float b0, float b1, float b2) {
  float s = a0 * b0;
  s += a1 * b1;
  s += a2 * b2;
  return s;
}

// MatrixBase::norm (`Pc.norm()`, `PO.norm()`, Frame.cc:614, 636): sqrtf of squaredNorm
RGBL_HD float fr_norm(float a0, float a1, float a2) {
#if defined(__HIP_DEVICE_COMPILE__)
  // Correctly rounded whatever the compiler's switches: the fp64 square root is IEEE, and rounding it to fp32 equals the
  // correctly rounded fp32 root (53 >= 2 * 24 + 2 bits).  NOT __fsqrt_rn: HIP maps it to the native, 1-ulp instruction
  // unless OCML_BASIC_ROUNDED_OPERATIONS is defined - measured on the MI355X: 3 of 63 depths one ulp off.
  return (float)sqrt((double)fr_dot(a0, a1, a2, a0, a1, a2));
#else
  return sqrtf(fr_dot(a0, a1, a2, a0, a1, a2));
#endif
}

// Vector / scalar and scalar / scalar (`normali / normali.norm()`, `normal / n`, `mfMaxDistance / mvScaleFactors[nLevels - 1]`,
// MapPoint.cc:457, 491-492): one IEEE fp32 division per component
RGBL_HD float fr_quot(float a, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the fp64 quotient is IEEE, and rounding it to fp32 equals the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits),
  // whatever the compiler's switches make of an fp32 division; 0 / 0 stays a NaN
  return (float)((double)a / (double)s);
#else
  return a / s;
#endif
}

}  // namespace rgbl
