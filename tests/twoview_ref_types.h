// Stand-in types for compiling the reference's own TwoViewReconstruction functions (src/TwoViewReconstruction.cc: the constructor,
// Reconstruct, FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography, CheckFundamental, ReconstructF,
// ReconstructH, Normalize, CheckRT, DecomposeE), cut out by signature at test time (tests/twoview_golden.py) and compiled
// UNMODIFIED against this header.  There is no Eigen here: every Eigen operation hands out the arithmetic of
// csrc/twoview_math.h - products of 3 x 3 matrices stay in fp64 from factor to factor and are rounded where they are assigned to a
// float matrix, JacobiSVD is tv_null_vector_rows / tv_svd3, inverse() is tv_inv3, norm() / dot() are fp64 rounded to float,
// GeometricTools::Triangulate is np_triangulate.  So this tier pins the reference's CONTROL FLOW, its plain-C++ arithmetic
// (Normalize, both Check* functions, the fp32 formulas of ReconstructH, CheckRT's tests, every integer rule) and its summation
// order - not Eigen's bits.  acos: the reference's unqualified call resolves, inside namespace ORB_SLAM3, to the overload set
// below, which mirrors std's (float, double, long double) and counts which one is bound.
#pragma once
#include <math.h>
#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <iostream>
#include <thread>
#include <utility>
#include <vector>

#include "twoview_math.h"
#include "Random.h"

#define CV_PI 3.1415926535897932384626433832795
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW

namespace cv {
struct Point2f { float x = 0, y = 0; Point2f() {} Point2f(float a, float b) : x(a), y(b) {} };
struct Point3f { float x = 0, y = 0, z = 0; Point3f() {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct KeyPoint { Point2f pt; };
}  // namespace cv

namespace Eigen {
enum { ComputeFullU = 1, ComputeFullV = 2, RowMajor = 1, ColMajor = 0 };

struct Matrix3f;
// a 3 x 3 in fp64: an Eigen product on its way, or a factor of a JacobiSVD
struct MatD3 {
  double m[9];
  MatD3 transpose() const { MatD3 r; rgbl::tv_transpose3(m, r.m); return r; }
};
struct VecD3 { double v[3]; };
struct Vector3f {
  float v[3] = {0, 0, 0};
  Vector3f() {}
  Vector3f(float a, float b, float c) { v[0] = a; v[1] = b; v[2] = c; }
  Vector3f(const VecD3& d) { for (int i = 0; i < 3; ++i) v[i] = (float)d.v[i]; }
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
  void setZero() { v[0] = v[1] = v[2] = 0.f; }
  Vector3f operator-() const { return Vector3f(-v[0], -v[1], -v[2]); }
  Vector3f operator-(const Vector3f& o) const { return Vector3f(v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]); }
  Vector3f& operator*=(float s) { for (int i = 0; i < 3; ++i) v[i] = v[i] * s; return *this; }
  float norm() const { const double x = v[0], y = v[1], z = v[2]; return (float)sqrt((x * x + y * y) + z * z); }
  float dot(const Vector3f& o) const { return (float)(((double)v[0] * (double)o.v[0] + (double)v[1] * (double)o.v[1]) + (double)v[2] * (double)o.v[2]); }
  Vector3f operator/(float s) const { return Vector3f((float)((double)v[0] / (double)s), (float)((double)v[1] / (double)s), (float)((double)v[2] / (double)s)); }
};
inline VecD3 operator+(const VecD3& a, const Vector3f& b) { VecD3 r; for (int i = 0; i < 3; ++i) r.v[i] = a.v[i] + (double)b.v[i]; return r; }

template <class S, int N> struct DiagonalMatrix {
  float d[3];
  explicit DiagonalMatrix(const Vector3f& w) { for (int i = 0; i < 3; ++i) d[i] = w(i); }
};

struct Matrix3f {
  float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  Matrix3f() {}
  Matrix3f(const MatD3& d) { rgbl::tv_round3(d.m, m); }
  float& operator()(int r, int c) { return m[3 * r + c]; }
  float operator()(int r, int c) const { return m[3 * r + c]; }
  void setZero() { for (int i = 0; i < 9; ++i) m[i] = 0.f; }
  MatD3 widen() const { MatD3 r; rgbl::tv_widen3(m, r.m); return r; }
  Matrix3f transpose() const { Matrix3f r; for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.m[3 * i + j] = m[3 * j + i]; return r; }
  Matrix3f inverse() const { MatD3 a = widen(), b; rgbl::tv_inv3(a.m, b.m); return Matrix3f(b); }
  double determinant() const { MatD3 a = widen(); return rgbl::ml_det3(a.m); }
  Matrix3f operator-() const { Matrix3f r; for (int i = 0; i < 9; ++i) r.m[i] = -m[i]; return r; }
  Vector3f col(int c) const { return Vector3f(m[c], m[3 + c], m[6 + c]); }
};
inline MatD3 mul(const MatD3& a, const MatD3& b) { MatD3 r; rgbl::tv_mul3(a.m, b.m, r.m); return r; }
inline MatD3 operator*(const Matrix3f& a, const Matrix3f& b) { return mul(a.widen(), b.widen()); }
inline MatD3 operator*(const MatD3& a, const Matrix3f& b) { return mul(a, b.widen()); }
inline MatD3 operator*(const MatD3& a, const MatD3& b) { return mul(a, b); }
inline MatD3 operator*(float s, const Matrix3f& a) { MatD3 r = a.widen(); for (int i = 0; i < 9; ++i) r.m[i] = (double)s * r.m[i]; return r; }
inline MatD3 operator*(const MatD3& a, const DiagonalMatrix<float, 3>& d) {
  MatD3 r;
  for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) r.m[3 * i + k] = a.m[3 * i + k] * (double)d.d[k];
  return r;
}
inline VecD3 operator*(const Matrix3f& a, const Vector3f& x) {
  MatD3 A = a.widen();
  const double xd[3] = {(double)x(0), (double)x(1), (double)x(2)};
  VecD3 r;
  rgbl::ml_matvec(A.m, xd, r.v);
  return r;
}

// Eigen::Matrix<float,3,3,RowMajor> built from a pointer (ComputeH21 / ComputeF21), Eigen::Matrix<float,3,4> (CheckRT)
template <class S, int R, int C, int O = ColMajor> struct Matrix;
template <int O> struct Matrix<float, 3, 3, O> {
  float m[9];
  explicit Matrix(const float* p) { for (int i = 0; i < 9; ++i) m[i] = p[i]; }   // row-major data
  operator Matrix3f() const { Matrix3f r; for (int i = 0; i < 9; ++i) r.m[i] = m[i]; return r; }
};
template <int O> struct Matrix<float, 3, 4, O> {
  float m[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  void setZero() { for (int i = 0; i < 12; ++i) m[i] = 0.f; }
  template <int BR, int BC> struct Block {
    Matrix* p; int r0, c0;
    void operator=(const Matrix3f& a) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) p->m[4 * (r0 + i) + c0 + j] = a(i, j); }
    void operator=(const Vector3f& a) { for (int i = 0; i < 3; ++i) p->m[4 * (r0 + i) + c0] = a(i); }
  };
  template <int BR, int BC> Block<BR, BC> block(int r, int c) { return Block<BR, BC>{this, r, c}; }
};
inline Matrix<float, 3, 4> operator*(const Matrix3f& K, const Matrix<float, 3, 4>& P) {
  Matrix<float, 3, 4> r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j)
      r.m[4 * i + j] = (float)(((double)K(i, 0) * (double)P.m[j] + (double)K(i, 1) * (double)P.m[4 + j]) + (double)K(i, 2) * (double)P.m[8 + j]);
  return r;
}

struct MatrixXf {
  int rows, cols;
  std::vector<float> a;
  MatrixXf(int r, int c) : rows(r), cols(c), a((size_t)r * c, 0.f) {}
  float& operator()(int r, int c) { return a[(size_t)r * cols + c]; }
  float operator()(int r, int c) const { return a[(size_t)r * cols + c]; }
};

template <class M> struct JacobiSVD;
template <> struct JacobiSVD<MatrixXf> {
  float h[9];
  struct V { const float* h; struct Col { const float* h; const float* data() const { return h; } }; Col col(int) const { return Col{h}; } };
  JacobiSVD(const MatrixXf& A, int) {
    static thread_local rgbl::TvWork work;   // FindHomography and FindFundamental run on two threads
    rgbl::TvHostX x;
    for (int r = 0; r < A.rows; ++r) for (int c = 0; c < 9; ++c) work.rows[r][c] = (double)A(r, c);
    rgbl::tv_null_vector_rows(x, work, A.rows, h);
  }
  V matrixV() const { return V{h}; }   // only col(8) is read
};
template <> struct JacobiSVD<Matrix3f> {
  MatD3 U, Vm;
  double w[3];
  JacobiSVD(const Matrix3f& A, int) { MatD3 a = A.widen(); rgbl::tv_svd3(a.m, U.m, w, Vm.m); }
  MatD3 matrixU() const { return U; }
  MatD3 matrixV() const { return Vm; }
  Vector3f singularValues() const { return Vector3f((float)w[0], (float)w[1], (float)w[2]); }
};
}  // namespace Eigen

namespace Sophus {
struct SE3f {
  Eigen::Matrix3f R;
  Eigen::Vector3f t;
  bool assigned = false;
  SE3f() {}
  SE3f(const Eigen::Matrix3f& r, const Eigen::Vector3f& tt) : R(r), t(tt), assigned(true) {}
};
}  // namespace Sophus

namespace ORB_SLAM3 {
// which acos the call at :895 binds
extern int g_acos_float, g_acos_double;
inline float acos(float x) { ++g_acos_float; return rgbl::tv_acosf(x); }
inline double acos(double x) { ++g_acos_double; return rgbl::ml_acos(x); }
inline long double acos(long double x) { ++g_acos_double; return (long double)rgbl::ml_acos((double)x); }

struct GeometricTools {
  // GeometricTools::Triangulate by np_triangulate; where it returns false the reference leaves x3D uninitialised and CheckRT reads it:
  // NaN here, which CheckRT's isfinite test skips - the deviation csrc/twoview_math.h states
  static bool Triangulate(Eigen::Vector3f& x_c1, Eigen::Vector3f& x_c2, Eigen::Matrix<float, 3, 4>& T1, Eigen::Matrix<float, 3, 4>& T2, Eigen::Vector3f& x3D) {
    const float a[2] = {x_c1(0), x_c1(1)}, b[2] = {x_c2(0), x_c2(1)};
    float X[3];
    if (!rgbl::np_triangulate(a, b, T1.m, T2.m, X)) { x3D = Eigen::Vector3f(NAN, NAN, NAN); return false; }
    x3D = Eigen::Vector3f(X[0], X[1], X[2]);
    return true;
  }
};

// the class as include/TwoViewReconstruction.h declares it; everything public for the glue
class TwoViewReconstruction {
 public:
  typedef std::pair<int, int> Match;
  TwoViewReconstruction(const Eigen::Matrix3f& k, float sigma = 1.0, int iterations = 200);
  bool Reconstruct(const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2, const std::vector<int>& vMatches12, Sophus::SE3f& T21,
                   std::vector<cv::Point3f>& vP3D, std::vector<bool>& vbTriangulated);
  void FindHomography(std::vector<bool>& vbMatchesInliers, float& score, Eigen::Matrix3f& H21);
  void FindFundamental(std::vector<bool>& vbInliers, float& score, Eigen::Matrix3f& F21);
  Eigen::Matrix3f ComputeH21(const std::vector<cv::Point2f>& vP1, const std::vector<cv::Point2f>& vP2);
  Eigen::Matrix3f ComputeF21(const std::vector<cv::Point2f>& vP1, const std::vector<cv::Point2f>& vP2);
  float CheckHomography(const Eigen::Matrix3f& H21, const Eigen::Matrix3f& H12, std::vector<bool>& vbMatchesInliers, float sigma);
  float CheckFundamental(const Eigen::Matrix3f& F21, std::vector<bool>& vbMatchesInliers, float sigma);
  bool ReconstructF(std::vector<bool>& vbMatchesInliers, Eigen::Matrix3f& F21, Eigen::Matrix3f& K, Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated);
  bool ReconstructH(std::vector<bool>& vbMatchesInliers, Eigen::Matrix3f& H21, Eigen::Matrix3f& K, Sophus::SE3f& T21, std::vector<cv::Point3f>& vP3D,
                    std::vector<bool>& vbTriangulated, float minParallax, int minTriangulated);
  void Normalize(const std::vector<cv::KeyPoint>& vKeys, std::vector<cv::Point2f>& vNormalizedPoints, Eigen::Matrix3f& T);
  int CheckRT(const Eigen::Matrix3f& R, const Eigen::Vector3f& t, const std::vector<cv::KeyPoint>& vKeys1, const std::vector<cv::KeyPoint>& vKeys2,
              const std::vector<Match>& vMatches12, std::vector<bool>& vbMatchesInliers, const Eigen::Matrix3f& K, std::vector<cv::Point3f>& vP3D, float th2,
              std::vector<bool>& vbGood, float& parallax);
  void DecomposeE(const Eigen::Matrix3f& E, Eigen::Matrix3f& R1, Eigen::Matrix3f& R2, Eigen::Vector3f& t);

  std::vector<cv::KeyPoint> mvKeys1, mvKeys2;
  std::vector<Match> mvMatches12;
  std::vector<bool> mvbMatched1;
  Eigen::Matrix3f mK;
  float mSigma, mSigma2;
  int mMaxIterations;
  std::vector<std::vector<size_t> > mvSets;
};
}  // namespace ORB_SLAM3
