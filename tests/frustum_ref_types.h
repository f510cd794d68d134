// frustum_ref_types.h — stand-in Frame / MapPoint / Pinhole declarations for the bodies of the reference's
// Frame::isInFrustum, MapPoint::PredictScale(const float&, Frame*), MapPoint::Get{Min,Max}DistanceInvariance and
// Pinhole::project(const Eigen::Vector3f&), which tests/frustum_golden.py cuts out of the reference's sources by signature
// at test time (into the build directory) and tests/frustum_ref_glue.cpp compiles unmodified.  Only the members those five
// bodies touch.  Eigen comes from the stand-in oracle/cvcompat/sophus/sim3.hpp (read-only): it defines the operation order
// the device kernel follows.  TEST INFRASTRUCTURE.
#pragma once
#include <math.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "sophus/sim3.hpp"

namespace Eigen {
// Eigen::Matrix<float, 3, 1> / <float, 3, 3> as the reference spells them in Frame.cc
template <class T, int R, int C> struct MatrixOf;
template <> struct MatrixOf<float, 3, 1> { typedef Vec<3> type; };
template <> struct MatrixOf<float, 2, 1> { typedef Vec<2> type; };
template <> struct MatrixOf<float, 3, 3> { typedef Matrix3f type; };
template <class T, int R, int C> using Matrix = typename MatrixOf<T, R, C>::type;
}  // namespace Eigen

namespace ORB_SLAM3 {
using namespace std;   // the reference's sources name unique_lock, mutex, log and ceil unqualified

class Frame;
class KeyFrame;

class Pinhole {
 public:
  std::vector<float> mvParameters;   // fx, fy, cx, cy
  Eigen::Vector2f project(const Eigen::Vector3f& v3D);
};

class MapPoint {
 public:
  Eigen::Vector3f GetWorldPos() { return mWorldPos; }
  Eigen::Vector3f GetNormal() { return mNormalVector; }
  float GetMinDistanceInvariance();
  float GetMaxDistanceInvariance();
  int PredictScale(const float& currentDist, Frame* pF);
  // what isInFrustum writes; the stale values show what it leaves alone
  float mTrackProjX = -7, mTrackProjY = -7, mTrackDepth = -7, mTrackDepthR = -7, mTrackProjXR = -7, mTrackProjYR = -7;
  bool mbTrackInView = true, mbTrackInViewR = true;
  int mnTrackScaleLevel = -7, mnTrackScaleLevelR = -7;
  float mTrackViewCos = -7, mTrackViewCosR = -7;
  Eigen::Vector3f mWorldPos, mNormalVector;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexPos;
};

class Frame {
 public:
  bool isInFrustum(MapPoint* pMP, float viewingCosLimit);
  bool isInFrustumChecks(MapPoint*, float, bool bRight = false) { (void)bRight; return false; }   // the two-camera branch: never reached (Nleft == -1)
  int Nleft = -1;
  Pinhole* mpCamera = nullptr;
  float mbf = 0;
  int mnScaleLevels = 0;
  float mfLogScaleFactor = 0;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  Eigen::Matrix<float, 3, 1> mOw;
  Eigen::Matrix<float, 3, 3> mRcw;
  Eigen::Matrix<float, 3, 1> mtcw;
};

}  // namespace ORB_SLAM3
