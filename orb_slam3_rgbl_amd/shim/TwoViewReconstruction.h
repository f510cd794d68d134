// TwoViewReconstruction.h — drop-in for ORB_SLAM3::TwoViewReconstruction (include/TwoViewReconstruction.h,
// src/TwoViewReconstruction.cc) with every homography and fundamental hypothesis of a call evaluated on the device: Reconstruct
// is ONE rgbl_two_view_reconstruct call.  INTEGRATION.md shows the lines of Pinhole::ReconstructWithTwoViews that change.
//
//   typedef rgbl_shim::TwoViewReconstruction<Eigen::Matrix3f, Eigen::Vector3f, Sophus::SE3f, cv::KeyPoint, cv::Point3f> TwoViewReconstruction;
//
// Matrix3T / Vector3T need a default constructor and operator()(row, col) / operator()(i); SE3T the constructor (Matrix3T,
// Vector3T); KeyPointT the member pt with x and y; Point3T the constructor (float, float, float).
//
// What stays on the host, as in the reference: mvMatches12 (:55-64) and the drawing of mvSets (:78-98).  The sets are drawn by
// DUtils::Random::RandomInt's formula (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) over glibc's rand() algorithm (random_r,
// TYPE_3) with a state of THIS header's own, seeded once per process as DUtils::Random::SeedRandOnce(0) seeds rand() (:81:
// srand(0), which glibc treats as srand(1)).  The reference draws from the process-wide rand(): its stream is this one as long
// as nothing else in the process calls rand() in between.
//
// vP3D: ReconstructH never assigns it - bestP3D is dropped at :725-731 - so on the homography path the reference returns true
// with the caller's vector untouched, and so does this class.  assign_p3d_on_homography = true (off by default) assigns the
// winning hypothesis's points there too.
#pragma once
#include <stdint.h>

#include <iostream>
#include <mutex>
#include <vector>

#include "rgbl_frontend.h"

namespace rgbl_shim {

// glibc's rand() (stdlib/random_r.c, TYPE_3: r[i] = r[i - 3] + r[i - 31], the result shifted right by one)
class GlibcRand {
 public:
  explicit GlibcRand(unsigned seed) {
    if (seed == 0) seed = 1;
    int32_t r[34];
    r[0] = (int32_t)seed;
    for (int i = 1; i < 31; ++i) {
      const long hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
      long word = 16807 * lo - 2836 * hi;
      if (word < 0) word += 2147483647;
      r[i] = (int32_t)word;
    }
    for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
    for (int i = 0; i < 31; ++i) s_[i] = (uint32_t)r[3 + i];
    at_ = 0;
    for (int i = 0; i < 310; ++i) step();
  }
  int rand() { return (int)(step() >> 1); }
  // DUtils::Random::RandomInt
  int RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)2147483647 + 1.0)) * d) + min;
  }

 private:
  uint32_t step() {   // s_[at_] is r[i - 31], s_[at_ + 28] is r[i - 3]
    const uint32_t v = s_[at_] + s_[(at_ + 28) % 31];
    s_[at_] = v;
    at_ = (at_ + 1) % 31;
    return v;
  }
  uint32_t s_[31];
  int at_;
};

template <class Matrix3T, class Vector3T, class SE3T, class KeyPointT, class Point3T>
class TwoViewReconstruction {
 public:
  TwoViewReconstruction(const Matrix3T& k, float sigma = 1.0, int iterations = 200, bool assign_p3d_on_homography = false, int device = 0)
      : mSigma(sigma), mMaxIterations(iterations), mbAssignOnH(assign_p3d_on_homography), mnDevice(device) {
    mK[0] = k(0, 0); mK[1] = k(1, 1); mK[2] = k(0, 2); mK[3] = k(1, 2);
  }

  bool Reconstruct(const std::vector<KeyPointT>& vKeys1, const std::vector<KeyPointT>& vKeys2, const std::vector<int>& vMatches12, SE3T& T21,
                   std::vector<Point3T>& vP3D, std::vector<bool>& vbTriangulated) {
    const int n1 = (int)vKeys1.size(), n2 = (int)vKeys2.size();
    std::vector<float> xy1(2 * (size_t)n1), xy2(2 * (size_t)n2);
    for (int i = 0; i < n1; ++i) { xy1[2 * (size_t)i] = vKeys1[(size_t)i].pt.x; xy1[2 * (size_t)i + 1] = vKeys1[(size_t)i].pt.y; }
    for (int i = 0; i < n2; ++i) { xy2[2 * (size_t)i] = vKeys2[(size_t)i].pt.x; xy2[2 * (size_t)i + 1] = vKeys2[(size_t)i].pt.y; }
    std::vector<int32_t> m12((size_t)n1, -1);
    int N = 0;
    for (size_t i = 0; i < vMatches12.size() && i < (size_t)n1; ++i)
      if (vMatches12[i] >= 0) { m12[i] = vMatches12[i]; ++N; }
    // mvSets (:78-98)
    mvSets.assign((size_t)(mMaxIterations > 0 ? mMaxIterations : 0) * 8, 0);
    if (N >= 8) {
      std::lock_guard<std::mutex> lock(RandMutex());
      std::vector<size_t> vAllIndices((size_t)N), vAvailableIndices;
      for (int i = 0; i < N; ++i) vAllIndices[(size_t)i] = (size_t)i;
      for (int it = 0; it < mMaxIterations; ++it) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; ++j) {
          const int randi = Rand().RandomInt(0, (int)vAvailableIndices.size() - 1);
          mvSets[8 * (size_t)it + j] = (int32_t)vAvailableIndices[(size_t)randi];
          vAvailableIndices[(size_t)randi] = vAvailableIndices.back();
          vAvailableIndices.pop_back();
        }
      }
    }
    rgbl_two_view_input in = {};
    rgbl_two_view_output out = {};
    in.n1 = n1; in.n2 = n2; in.kp1_xy = xy1.data(); in.kp2_xy = xy2.data(); in.matches12 = m12.data();
    for (int i = 0; i < 4; ++i) in.K[i] = mK[i];
    in.sigma = mSigma; in.n_hyp = mMaxIterations; in.samples = mvSets.data();
    std::vector<float> p3d(3 * (size_t)n1, 0.0f);
    std::vector<uint8_t> tri((size_t)n1, 0);
    out.p3d = p3d.data(); out.triangulated = tri.data();
    rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
    int rc = rgbl_matcher_acquire(mnDevice, &h);
    if (rc == RGBL_OK) {
      rc = rgbl_two_view_reconstruct(h, &in, &out);
      rgbl_matcher_release(h);
    }
    if (rc != RGBL_OK) {   // fewer than eight matches included: the reference would index an empty vector there
      std::cerr << "rgbl_shim::TwoViewReconstruction: " << rgbl_last_error() << std::endl;
      return false;
    }
    mLast = out;
    mLast.p3d = nullptr; mLast.triangulated = nullptr;
    if (!out.found) return false;
    Matrix3T R;
    Vector3T t;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) R(i, j) = out.R21[3 * i + j];
      t(i) = out.t21[i];
    }
    T21 = SE3T(R, t);
    vbTriangulated.assign((size_t)n1, false);
    for (int i = 0; i < n1; ++i) vbTriangulated[(size_t)i] = tri[(size_t)i] != 0;
    if (out.p3d_assigned || mbAssignOnH) {
      vP3D.clear();
      for (int i = 0; i < n1; ++i) vP3D.push_back(Point3T(p3d[3 * (size_t)i], p3d[3 * (size_t)i + 1], p3d[3 * (size_t)i + 2]));
    }
    return true;
  }

  // what the last Reconstruct computed (scores, winners, exit, n_good, parallax; the array pointers are null) and the sets it drew
  const rgbl_two_view_output& Last() const { return mLast; }
  const std::vector<int32_t>& Sets() const { return mvSets; }

 private:
  static GlibcRand& Rand() { static GlibcRand r(0); return r; }
  static std::mutex& RandMutex() { static std::mutex m; return m; }
  float mK[4], mSigma;
  int mMaxIterations;
  bool mbAssignOnH;
  int mnDevice;
  std::vector<int32_t> mvSets;
  rgbl_two_view_output mLast = {};
};

}  // namespace rgbl_shim
