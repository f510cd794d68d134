// sim3_ref_types.h — stand-in declarations for the reference's include/Sim3Solver.h and src/Sim3Solver.cc, which
// tests/sim3_golden.py copies at test time into the build directory without their #include lines, together with
// Pinhole::project(const Eigen::Vector3f&) cut out of src/CameraModels/Pinhole.cpp by signature, and tests/sim3_ref_glue.cpp
// compiles unmodified.  Only the members those bodies touch.  TEST INFRASTRUCTURE.
//
// This tier pins the reference's control flow: the constructor's bookkeeping, SetRansacParameters' iteration count, the
// drawing of the samples through the reference's own DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp, compiled
// beside it) over rand() after srand(seed), the `>=` and `>` rules, the mapping through mvnIndices1, the N < mRansacMinInliers
// exit, both overloads of iterate over repeated calls, the truncation of 9.210 * sigma2 in std::vector<size_t>.
// It does NOT pin:
//   - the eigen decomposition: the EigenSolver stand-in hands out csrc/sim3_math.h's s3_top_eigenvector as column 0, with
//     eigenvalues (1, 0, 0, 0), so that eval.maxCoeff picks it;
//   - atan2: the reference's `atan2(vec.norm(), evec(0, maxIndex))` has two float arguments and sits under a using-directive
//     for std, so with <cmath> it binds to std::atan2(float, float) and `double ang` receives a float; csrc/sim3_math.h follows
//     the declared type and evaluates its own s3_atan2 in fp64.  ORB_SLAM3::atan2 below hands out the header's, as for the
//     eigenvector, so what is compared is the control flow around it;
//   - Eigen's evaluation order: the operators below are written in the order csrc/sim3_math.h uses (sums left to right,
//     `(array * array).sum()` column by column, a double scalar rounded to float before it multiplies a float matrix);
//   - Sophus::SO3f::exp: the stand-in is the header's s3_so3_exp.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/csrc/sim3_math.h"

#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW

namespace Eigen {
struct Vector2f {
  float v[2] = {0, 0};
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  Vector2f operator-(const Vector2f& o) const { Vector2f r; r.v[0] = v[0] - o.v[0]; r.v[1] = v[1] - o.v[1]; return r; }
  float dot(const Vector2f& o) const { return v[0] * o.v[0] + v[1] * o.v[1]; }
};
struct Vector3f {
  float v[3] = {0, 0, 0};
  Vector3f() {}
  Vector3f(float a, float b, float c) { v[0] = a; v[1] = b; v[2] = c; }
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  Vector3f operator-(const Vector3f& o) const { return Vector3f(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
  Vector3f operator+(const Vector3f& o) const { return Vector3f(v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]); }
  Vector3f operator/(float s) const { return Vector3f(v[0] / s, v[1] / s, v[2] / s); }
  float norm() const { return rgbl::fr_norm(v[0], v[1], v[2]); }
};
inline Vector3f operator*(double s, const Vector3f& a) { const float f = (float)s; return Vector3f(f * a.v[0], f * a.v[1], f * a.v[2]); }
struct Vector4f {
  float v[4] = {0, 0, 0, 0};
  float maxCoeff(int* idx) const {
    int k = 0;
    for (int i = 1; i < 4; ++i) if (v[i] > v[k]) k = i;
    *idx = k;
    return v[k];
  }
};

// the glue sets this to see WHICH element of mvX3Dc1 the reference copies into a column of P3Dc1i: the triples it drew
inline void (*sim3_ref_on_column)(const Vector3f*) = nullptr;

struct Array33 {
  float a[9];   // column by column
  Array33 operator*(const Array33& o) const { Array33 r; for (int k = 0; k < 9; ++k) r.a[k] = a[k] * o.a[k]; return r; }
  float sum() const { float s = 0.0f; for (int k = 0; k < 9; ++k) s += a[k]; return s; }
};
template <class T, int R, int C> using Array = Array33;

struct Matrix3f {
  float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // row-major
  float& operator()(int i, int j) { return m[3 * i + j]; }
  float operator()(int i, int j) const { return m[3 * i + j]; }
  struct ColRef {
    Matrix3f* p; int j;
    void operator=(const Vector3f& x) {
      if (sim3_ref_on_column) sim3_ref_on_column(&x);
      for (int i = 0; i < 3; ++i) p->m[3 * i + j] = x.v[i];
    }
    Vector3f operator-(const Vector3f& c) const { return Vector3f(p->m[j] - c.v[0], p->m[3 + j] - c.v[1], p->m[6 + j] - c.v[2]); }
  };
  ColRef col(int j) { return ColRef{this, j}; }
  struct RowWise {
    const Matrix3f* p;
    Vector3f sum() const { return Vector3f((p->m[0] + p->m[1]) + p->m[2], (p->m[3] + p->m[4]) + p->m[5], (p->m[6] + p->m[7]) + p->m[8]); }
  };
  RowWise rowwise() const { return RowWise{this}; }
  int cols() const { return 3; }
  Matrix3f transpose() const { Matrix3f r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[3 * i + j] = m[3 * j + i]; return r; }
  Matrix3f operator*(const Matrix3f& o) const {
    Matrix3f r;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.m[3 * i + j] = rgbl::fr_dot(m[3 * i], m[3 * i + 1], m[3 * i + 2], o.m[j], o.m[3 + j], o.m[6 + j]);
    return r;
  }
  Vector3f operator*(const Vector3f& x) const {
    return Vector3f(rgbl::fr_row_times(m, x.v[0], x.v[1], x.v[2]), rgbl::fr_row_times(m + 3, x.v[0], x.v[1], x.v[2]), rgbl::fr_row_times(m + 6, x.v[0], x.v[1], x.v[2]));
  }
  Matrix3f operator-() const { Matrix3f r; for (int k = 0; k < 9; ++k) r.m[k] = -m[k]; return r; }
  Array33 array() const { Array33 r; for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) r.a[3 * j + i] = m[3 * i + j]; return r; }
};
inline Matrix3f operator*(float s, const Matrix3f& a) { Matrix3f r; for (int k = 0; k < 9; ++k) r.m[k] = s * a.m[k]; return r; }
inline Matrix3f operator*(double s, const Matrix3f& a) { return (float)s * a; }

struct Matrix4f {
  float m[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // row-major; the reference leaves a fresh one uninitialised
  float& operator()(int i, int j) { return m[4 * i + j]; }
  float operator()(int i, int j) const { return m[4 * i + j]; }
  void setIdentity() { for (int k = 0; k < 16; ++k) m[k] = k % 5 == 0 ? 1.0f : 0.0f; }
  static Matrix4f Identity() { Matrix4f r; r.setIdentity(); return r; }
  struct Comma {
    float* p;
    Comma operator,(double x) { *p = (float)x; return Comma{p + 1}; }
  };
  Comma operator<<(double x) { m[0] = (float)x; return Comma{m + 1}; }
  template <int R, int C> struct BlockRef {
    Matrix4f* p; int i0, j0;
    void operator=(const Matrix3f& a) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p->m[4 * (i0 + i) + j0 + j] = a.m[3 * i + j]; }
    void operator=(const Vector3f& a) { for (int i = 0; i < 3; ++i) p->m[4 * (i0 + i) + j0] = a.v[i]; }
    operator Matrix3f() const { Matrix3f a; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) a.m[3 * i + j] = p->m[4 * (i0 + i) + j0 + j]; return a; }
    operator Vector3f() const { return Vector3f(p->m[4 * i0 + j0], p->m[4 * (i0 + 1) + j0], p->m[4 * (i0 + 2) + j0]); }
  };
  template <int R, int C> BlockRef<R, C> block(int i, int j) { return BlockRef<R, C>{this, i, j}; }
};

template <class M> struct EigenSolver {
  Vector4f values;
  Matrix4f vectors;
  struct Values { Vector4f v; Vector4f real() const { return v; } };
  struct Vectors { Matrix4f v; Matrix4f real() const { return v; } };
  void compute(const Matrix4f& N) {
    const float n[10] = {N(0, 0), N(0, 1), N(0, 2), N(0, 3), N(1, 1), N(1, 2), N(1, 3), N(2, 2), N(2, 3), N(3, 3)};
    float e[4];
    rgbl::s3_top_eigenvector(n, e);
    vectors = Matrix4f();
    for (int i = 0; i < 4; ++i) vectors(i, 0) = e[i];
    values = Vector4f();
    values.v[0] = 1.0f;
  }
  Values eigenvalues() const { return Values{values}; }
  Vectors eigenvectors() const { return Vectors{vectors}; }
};
}  // namespace Eigen

namespace Sophus {
struct SO3f {
  Eigen::Matrix3f R;
  static SO3f exp(const Eigen::Vector3f& om) { SO3f r; rgbl::s3_so3_exp(om.v, r.R.m); return r; }
  Eigen::Matrix3f matrix() const { return R; }
};
}  // namespace Sophus

namespace cv {
struct KeyPoint { int octave = 0; };
}  // namespace cv

#include "Random.h"   // the reference's own Thirdparty/DBoW2/DUtils/Random.h (on the include path of the build); Random.cpp beside it

namespace ORB_SLAM3 {
using namespace std;   // the reference's sources name vector, max, min, get, abs, ceil, log, pow unqualified

#ifndef SIM3_REF_STD_ATAN2   // defined: the call binds as in the reference, to std::atan2(float, float) (to measure the difference)
inline double atan2(float y, float x) { return rgbl::s3_atan2((double)y, (double)x); }   // see the head of this file
#endif

struct CvMat33 {
  float a[9];
  double dot(const CvMat33& o) const { double s = 0; for (int k = 0; k < 9; ++k) s += (double)a[k] * (double)o.a[k]; return s; }
};
struct Converter {
  static CvMat33 toCvMat(const Eigen::Matrix3f& M) { CvMat33 r; for (int k = 0; k < 9; ++k) r.a[k] = M.m[k]; return r; }
};

class GeometricCamera {
 public:
  virtual ~GeometricCamera() {}
  virtual Eigen::Vector2f project(const Eigen::Vector3f& v3D) = 0;
};
class Pinhole : public GeometricCamera {
 public:
  std::vector<float> mvParameters;   // fx, fy, cx, cy
  Eigen::Vector2f project(const Eigen::Vector3f& v3D);
};

class KeyFrame;
class MapPoint {
 public:
  Eigen::Vector3f pos;
  bool bad = false;
  KeyFrame* kf = nullptr;   // the key frame that observes it ...
  int index = -1;           // ... at this feature
  bool isBad() { return bad; }
  std::tuple<int, int> GetIndexInKeyFrame(KeyFrame* p) { return p == kf ? std::make_tuple(index, -1) : std::make_tuple(-1, -1); }
  Eigen::Vector3f GetWorldPos() { return pos; }
};
class KeyFrame {
 public:
  GeometricCamera* mpCamera = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvLevelSigma2;
  Eigen::Matrix3f R;
  Eigen::Vector3f t;
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  Eigen::Matrix3f GetRotation() { return R; }
  Eigen::Vector3f GetTranslation() { return t; }
};
}  // namespace ORB_SLAM3
