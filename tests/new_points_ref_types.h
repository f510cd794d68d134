// new_points_ref_types.h — stand-in declarations for the bodies of the reference's LocalMapping::CreateNewMapPoints,
// GeometricTools::Triangulate, KeyFrame::UnprojectStereo, Pinhole::unprojectEig and Pinhole::project(cv::Point3f), which
// tests/new_points_golden.py cuts out of the reference's sources by signature at test time (into the build directory) and
// tests/new_points_ref_glue.cpp compiles unmodified.  Only the members those five bodies touch.
// Eigen / Sophus: the stand-in oracle/cvcompat/sophus/sim3.hpp (read-only; it defines the operation order the device follows),
// extended here by what these bodies use besides: Matrix<float,3,4> / Matrix4f with block<>, row().dot, Vector4f with head, and
// a JacobiSVD that hands out csrc/newpoint_math.h's null vector - so this tier pins the control flow, the overload resolution of
// cos / atan2 and the order of the tests, NOT the SVD or Eigen's evaluation order.  TEST INFRASTRUCTURE.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <list>
#include <mutex>
#include <utility>
#include <vector>

#define SE3 SE3Core   // Sophus::SE3<float> gets matrix3x4() below
#include "sophus/sim3.hpp"
#undef SE3

#include "../orb_slam3_rgbl_amd/csrc/newpoint_math.h"

namespace cv {
struct Point2f { float x = 0, y = 0; Point2f() {} Point2f(float a, float b) : x(a), y(b) {} };
struct Point3f { float x = 0, y = 0, z = 0; Point3f() {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct KeyPoint { Point2f pt; int octave = 0; float angle = 0; };
}  // namespace cv

namespace Eigen {
struct Row4 {
  float v[4];
  Row4 operator-(const Row4& o) const { Row4 r; for (int i = 0; i < 4; ++i) r.v[i] = v[i] - o.v[i]; return r; }
};
inline Row4 operator*(float s, const Row4& a) { Row4 r; for (int i = 0; i < 4; ++i) r.v[i] = s * a.v[i]; return r; }
struct Vector4f {
  float v[4];
  float operator()(int i) const { return v[i]; }
  Vector3f head(int) const { return Vector3f(v[0], v[1], v[2]); }
};
struct Mat33 : Matrix3f {
  Mat33() {}
  Mat33(const Matrix3f& o) : Matrix3f(o) {}
  Vector3f row(int i) const { return Vector3f(m[3 * i], m[3 * i + 1], m[3 * i + 2]); }
};
struct Mat34 {
  float m[12];   // row-major
  template <int R, int C> auto block(int i, int j) const {
    if constexpr (R == 3) {
      Mat33 r;
      for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) r.m[3 * a + b] = m[4 * (i + a) + j + b];
      return r;
    } else {
      Row4 r;
      for (int b = 0; b < 4; ++b) r.v[b] = m[4 * i + j + b];
      return r;
    }
  }
};
struct Matrix4f {
  float m[16];
  struct RowRef { float* p; void operator=(const Row4& r) { for (int i = 0; i < 4; ++i) p[i] = r.v[i]; } };
  template <int R, int C> RowRef block(int i, int) { return RowRef{m + 4 * i}; }
};
enum { ComputeFullV = 1 };
template <class M> struct JacobiSVD {
  struct V { Vector4f h; Vector4f col(int) const { return h; } } v_;
  JacobiSVD(const M& A, int) { rgbl::np_null_vector(A.m, v_.h.v); }
  const V& matrixV() const { return v_; }
};
template <class T, int R, int C> struct MatrixOf;
template <> struct MatrixOf<float, 3, 1> { typedef Vec<3> type; };
template <> struct MatrixOf<float, 3, 3> { typedef Mat33 type; };
template <> struct MatrixOf<float, 3, 4> { typedef Mat34 type; };
template <class T, int R, int C> using Matrix = typename MatrixOf<T, R, C>::type;
}  // namespace Eigen

namespace Sophus {
template <class T> class SE3;
template <> class SE3<float> : public SE3Core<float> {
 public:
  SE3() {}
  SE3(const SE3Core<float>& o) : SE3Core<float>(o) {}
  Eigen::Mat34 matrix3x4() const {
    Eigen::Mat34 r;
    const Eigen::Matrix3f R = rotationMatrix();
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) r.m[4 * i + j] = R(i, j); r.m[4 * i + 3] = translation()(i); }
    return r;
  }
};
}  // namespace Sophus

namespace ORB_SLAM3 {
using namespace std;   // the reference's sources name vector, min, cos, atan2, find, unique_lock unqualified

class KeyFrame;
class Map { public: bool GetIniertialBA2() { return false; } };

class GeometricCamera {
 public:
  virtual ~GeometricCamera() {}
  virtual cv::Point2f project(const cv::Point3f& p3D) = 0;
  virtual Eigen::Vector3f unprojectEig(const cv::Point2f& p2D) = 0;
};
class Pinhole : public GeometricCamera {
 public:
  std::vector<float> mvParameters;   // fx, fy, cx, cy
  cv::Point2f project(const cv::Point3f& p3D);
  Eigen::Vector3f unprojectEig(const cv::Point2f& p2D);
};

class MapPoint {
 public:
  MapPoint(const Eigen::Vector3f& Pos, KeyFrame* pRefKF, Map*) : mWorldPos(Pos), mpRefKF(pRefKF) {}
  void AddObservation(KeyFrame* pKF, int idx) { mObs.push_back(std::make_pair(pKF, idx)); }
  void ComputeDistinctiveDescriptors() {}
  void UpdateNormalAndDepth() {}
  Eigen::Vector3f mWorldPos;
  KeyFrame* mpRefKF;
  std::vector<std::pair<KeyFrame*, int> > mObs;
};

class KeyFrame {
 public:
  int index = -1;   // position among the neighbours (the glue's bookkeeping)
  int N = 0, NLeft = -1;
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mb = 0, mbf = 0, mfScaleFactor = 0, median_depth = 0;
  GeometricCamera* mpCamera = nullptr;
  GeometricCamera* mpCamera2 = nullptr;
  KeyFrame* mPrevKF = nullptr;
  std::vector<cv::KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
  std::vector<float> mvuRight, mvDepth, mvScaleFactors, mvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<KeyFrame*> neighbours;
  Sophus::SE3<float> mTcw, mTwc;
  Eigen::Matrix3f mRwc;
  std::mutex mMutexPose;
  Map map;
  Sophus::SE3<float> GetPose() { return mTcw; }
  Sophus::SE3<float> GetRightPose() { return mTcw; }
  Eigen::Vector3f GetCameraCenter() { return mTwc.translation(); }
  Eigen::Vector3f GetRightCameraCenter() { return mTwc.translation(); }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) { (void)n; return neighbours; }
  float ComputeSceneMedianDepth(const int) { return median_depth; }
  bool UnprojectStereo(int i, Eigen::Vector3f& x3D);
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
  Map* GetMap() { return &map; }
};

// ORBmatcher::SearchForTriangulation is the reference's own ORBmatcher.cc, reached through oracle/_ref/libref_orbmatcher.so
// (new_points_ref_glue.cpp flattens the two key frames for its entry point)
class ORBmatcher {
 public:
  ORBmatcher(float, bool) {}
  int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t> >& vMatchedPairs, const bool bOnlyStereo,
                             const bool bCoarse = false);
};

class Tracking { public: enum eTrackingState { OK = 2, RECENTLY_LOST = 3 }; int mState = OK; };
class Atlas {
 public:
  Map map;
  std::vector<MapPoint*> added;
  Map* GetCurrentMap() { return &map; }
  void AddMapPoint(MapPoint* pMP) { added.push_back(pMP); }
};
class GeometricTools {
 public:
  static bool Triangulate(Eigen::Vector3f& x_c1, Eigen::Vector3f& x_c2, Eigen::Matrix<float, 3, 4>& Tc1w, Eigen::Matrix<float, 3, 4>& Tc2w,
                          Eigen::Vector3f& x3D);
};
class LocalMapping {
 public:
  void CreateNewMapPoints();
  bool CheckNewKeyFrames() { return false; }
  bool mbMonocular = false, mbInertial = false, mbFarPoints = false;
  float mThFarPoints = 0;
  KeyFrame* mpCurrentKeyFrame = nullptr;
  Tracking* mpTracker = nullptr;
  Atlas* mpAtlas = nullptr;
  std::list<MapPoint*> mlpRecentAddedMapPoints;
};

}  // namespace ORB_SLAM3
