// logf_glibc.h — bit-faithful restatement of glibc 2.35 logf().
//
// Why: MapPoint::PredictScale (src/MapPoint.cc:531-546) evaluates `ceil(log(ratio) / mfLogScaleFactor)` on a float ratio,
// which binds to glibc's logf.  That function is NOT correctly rounded (≈0.82 ULP), so a device kernel predicts the same
// pyramid level as the CPU path only by evaluating the very same double-precision polynomial in the very same order.
// Algorithm: glibc sysdeps/ieee754/flt-32/e_logf.c (ARM optimized-routines logf, LOGF_TABLE_BITS = 4, degree-3 polynomial);
// table constants cross-checked against the bytes of __logf_data in this image's libm.so.6 (tests/test_logf_glibc.py,
// which also compares against the live libm over every float of [2^-12, 2^12]).
//
// Shared by the HIP kernels (device) and by CPU tests (host).  All arithmetic is IEEE double without FMA contraction
// (compile with -ffp-contract=off).
#pragma once
#include <stdint.h>

#ifndef RGBL_HD
#if defined(__HIPCC__)
#define RGBL_HD __host__ __device__ inline
#else
#define RGBL_HD inline
#endif
#endif

namespace rgbl {

RGBL_HD uint32_t lg_asuint(float f) {
  union { float f; uint32_t u; } c; c.f = f; return c.u;
}
RGBL_HD float lg_asfloat(uint32_t u) {
  union { float f; uint32_t u; } c; c.u = u; return c.f;
}

// __logf_data.tab[i] = {invc, logc}; a switch instead of an array: no constant-memory object in a header shared by
// several translation units, and the device compiler turns it into selects.
RGBL_HD void lg_table(int i, double* invc, double* logc) {
  switch (i) {
    case 0: *invc = 0x1.661ec79f8f3bep+0; *logc = -0x1.57bf7808caadep-2; break;
    case 1: *invc = 0x1.571ed4aaf883dp+0; *logc = -0x1.2bef0a7c06ddbp-2; break;
    case 2: *invc = 0x1.49539f0f010bp+0; *logc = -0x1.01eae7f513a67p-2; break;
    case 3: *invc = 0x1.3c995b0b80385p+0; *logc = -0x1.b31d8a68224e9p-3; break;
    case 4: *invc = 0x1.30d190c8864a5p+0; *logc = -0x1.6574f0ac07758p-3; break;
    case 5: *invc = 0x1.25e227b0b8eap+0; *logc = -0x1.1aa2bc79c81p-3; break;
    case 6: *invc = 0x1.1bb4a4a1a343fp+0; *logc = -0x1.a4e76ce8c0e5ep-4; break;
    case 7: *invc = 0x1.12358f08ae5bap+0; *logc = -0x1.1973c5a611cccp-4; break;
    case 8: *invc = 0x1.0953f419900a7p+0; *logc = -0x1.252f438e10c1ep-5; break;
    case 9: *invc = 0x1p+0; *logc = 0x0p+0; break;
    case 10: *invc = 0x1.e608cfd9a47acp-1; *logc = 0x1.aa5aa5df25984p-5; break;
    case 11: *invc = 0x1.ca4b31f026aap-1; *logc = 0x1.c5e53aa362eb4p-4; break;
    case 12: *invc = 0x1.b2036576afce6p-1; *logc = 0x1.526e57720db08p-3; break;
    case 13: *invc = 0x1.9c2d163a1aa2dp-1; *logc = 0x1.bc2860d22477p-3; break;
    case 14: *invc = 0x1.886e6037841edp-1; *logc = 0x1.1058bc8a07ee1p-2; break;
    default: *invc = 0x1.767dcf5534862p-1; *logc = 0x1.4043057b6ee09p-2; break;
  }
}

// glibc __logf.  Zero -> -inf, negative (and -0 is zero) -> NaN, +inf -> +inf, NaN -> NaN, subnormals are normalised first.
RGBL_HD float logf_glibc(float x) {
  const double ln2 = 0x1.62e42fefa39efp-1;
  const double a0 = -0x1.00ea348b88334p-2, a1 = 0x1.5575b0be00b6ap-2, a2 = -0x1.ffffef20a4123p-2;
  uint32_t ix = lg_asuint(x);
  if (ix == 0x3f800000u) return 0.f;
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
    // x < 0x1p-126 or inf or nan
    if (ix * 2u == 0u) return lg_asfloat(0xff800000u);                      // __math_divzerof(1): -inf
    if (ix == 0x7f800000u) return x;                                         // log(inf) == inf
    if ((ix & 0x80000000u) || ix * 2u >= 0xff000000u) return lg_asfloat(0x7fc00000u);  // __math_invalidf: NaN
    ix = lg_asuint(x * 0x1p23f);                                             // subnormal: normalise
    ix -= 23u << 23;
  }
  // x = 2^k z with z in [OFF, 2 OFF), split into 16 subintervals; invc is near 1 / (centre of the subinterval)
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (int)((tmp >> (23 - 4)) % 16u);
  const int k = (int32_t)tmp >> 23;  // arithmetic shift
  const uint32_t iz = ix - (tmp & 0xff800000u);
  double invc, logc;
  lg_table(i, &invc, &logc);
  const double z = (double)lg_asfloat(iz);
  // log(x) = log1p(z / c - 1) + log(c) + k ln2
  const double r = z * invc - 1;
  const double y0 = logc + (double)k * ln2;
  const double r2 = r * r;
  double y = a1 * r + a2;
  y = a0 * r2 + y;
  y = y * r2 + (y0 + r);
  return (float)y;
}

}  // namespace rgbl
