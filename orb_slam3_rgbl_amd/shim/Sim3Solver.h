// Sim3Solver.h — drop-in for ORB_SLAM3::Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) with the RANSAC on the device: a
// call of iterate is ONE rgbl_sim3_ransac call that evaluates every hypothesis the call may run.  INTEGRATION.md shows the
// lines of LoopClosing.cc that change.
//
//   typedef rgbl_shim::Sim3Solver<KeyFrame, Eigen::Matrix4f> Sim3Solver;
//
// Matrix4T needs a default constructor and operator()(row, col); the 3 x 3 and 3-vector types are what KeyFrame::GetRotation()
// and GetTranslation() return (operator()(row, col) / operator()(i)).  DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.h)
// must be declared before this header is included.
//
// What stays on the host, as in the reference: the constructor's bookkeeping (:35-121: isBad, GetIndexInKeyFrame, mvLevelSigma2,
// mvnIndices1, the camera-frame points), SetRansacParameters' iteration formula (:123-147), and the drawing of the samples with
// DUtils::Random::RandomInt and the swap-and-pop of vAvailableIndices (:172-186).  mnIterations, mnBestInliers and mBest*
// persist across calls.  The thresholds are what the reference STORES: mvnMaxError1 / 2 are std::vector<size_t>, so
// 9.210 * sigma2 is truncated to an integer (9 on level 0) before `err1 < mvnMaxError1[i]` converts it to float.
//
// Deviations from the reference:
//   - a call draws the triples of ALL the iterations it may run - min(nIterations, mRansacMaxIts - mnIterations) - before it
//     knows where the scan stops.  After a call that converged early the process-wide rand() stream is therefore further along
//     than the reference's; the call's own result is not affected (it uses the triples in the order drawn);
//   - the second overload of iterate returns an uninitialised bestSim3 when no iteration improves on mnBestInliers (zero
//     iterations run included); here it returns mBestT12 (the identity before any hypothesis was held);
//   - the eigen decomposition, atan2 and Eigen's evaluation order are this project's (csrc/sim3_math.h lists them).
//
// Pinhole cameras only: a key frame whose camera is not a Pinhole (GeometricCamera::CAM_PINHOLE) is refused with a message; every
// iterate then returns the identity with bNoMore = true, and SolveBatch returns false.
// With a DeviceLocalMap the points are read from the map points' slots (a point without one is uploaded on the spot), so the
// matches of rgbl_search_by_bow_keyframes need not leave the card.
#pragma once
#include <math.h>

#include <algorithm>
#include <iostream>
#include <memory>
#include <tuple>
#include <type_traits>
#include <vector>

#include "LocalMap.h"

namespace rgbl_shim {

template <class KeyFrameT, class Matrix4T>
class Sim3Solver {
 public:
  typedef typename std::decay<decltype(std::declval<KeyFrameT>().GetRotation())>::type Matrix3T;
  typedef typename std::decay<decltype(std::declval<KeyFrameT>().GetTranslation())>::type Vector3T;
  typedef typename std::remove_pointer<typename std::decay<decltype(std::declval<KeyFrameT>().GetMapPointMatches()[0])>::type>::type MapPointT;

  Sim3Solver(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true,
             std::vector<KeyFrameT*> vpKeyFrameMatchedMP = std::vector<KeyFrameT*>(), DeviceLocalMap* pMap = nullptr, int device = 0)
      : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale), mpMap(pMap), mnDevice(device) {
    SetIdentity(mBestT12);
    for (int i = 0; i < 3; ++i) {
      mBestTranslation(i) = 0.0f;
      for (int j = 0; j < 3; ++j) mBestRotation(i, j) = i == j ? 1.0f : 0.0f;
    }
    mBestScale = 1.0f;
    bool bDifferentKFs = false;
    if (vpKeyFrameMatchedMP.empty()) {
      bDifferentKFs = true;
      vpKeyFrameMatchedMP = std::vector<KeyFrameT*>(vpMatched12.size(), pKF2);
    }
    if (pKF1->mpCamera->GetType() != 0u || pKF2->mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) {
      std::cerr << "[Sim3Solver] only Pinhole cameras are covered by the device path" << std::endl;
      mbRefused = true;
    }
    std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    const Matrix3T Rcw1 = pKF1->GetRotation(), Rcw2 = pKF2->GetRotation();
    const Vector3T tcw1 = pKF1->GetTranslation(), tcw2 = pKF2->GetTranslation();
    for (int i = 0; i < 3; ++i) {
      mtcw1[i] = tcw1(i); mtcw2[i] = tcw2(i);
      for (int j = 0; j < 3; ++j) { mRcw1[3 * i + j] = Rcw1(i, j); mRcw2[3 * i + j] = Rcw2(i, j); }
    }
    for (int i = 0; i < 4; ++i) {
      mK1[i] = mbRefused ? 0.0f : pKF1->mpCamera->getParameter(i);
      mK2[i] = mbRefused ? 0.0f : pKF2->mpCamera->getParameter(i);
    }
    size_t idx = 0;
    KeyFrameT* pKFm = pKF2;
    for (int i1 = 0; i1 < mN1; i1++) {
      if (!vpMatched12[i1]) continue;
      MapPointT* pMP1 = vpKeyFrameMP1[i1];
      MapPointT* pMP2 = vpMatched12[i1];
      if (!pMP1) continue;
      if (pMP1->isBad() || pMP2->isBad()) continue;
      if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
      const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
      const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
      if (indexKF1 < 0 || indexKF2 < 0) continue;
      const float sigmaSquare1 = pKF1->mvLevelSigma2[pKF1->mvKeysUn[indexKF1].octave];
      const float sigmaSquare2 = pKFm->mvLevelSigma2[pKFm->mvKeysUn[indexKF2].octave];
      mvnMaxError1.push_back((float)(size_t)(9.210 * sigmaSquare1));   // std::vector<size_t> in the reference (:99-100)
      mvnMaxError2.push_back((float)(size_t)(9.210 * sigmaSquare2));
      mvpMapPoints1.push_back(pMP1);
      mvpMapPoints2.push_back(pMP2);
      mvnIndices1.push_back((size_t)i1);
      const Vector3T X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
      for (int r = 0; r < 3; ++r) {   // Rcw * Xw + tcw (:107, :110), products summed left to right as csrc/sim3_math.h does
        mvX3Dc1.push_back((mRcw1[3 * r] * X3D1w(0) + mRcw1[3 * r + 1] * X3D1w(1)) + mRcw1[3 * r + 2] * X3D1w(2) + mtcw1[r]);
        mvX3Dc2.push_back((mRcw2[3 * r] * X3D2w(0) + mRcw2[3 * r + 1] * X3D2w(1)) + mRcw2[3 * r + 2] * X3D2w(2) + mtcw2[r]);
      }
      mvAllIndices.push_back(idx);
      idx++;
    }
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = (int)mvpMapPoints1.size();
    float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) {
      nIterations = 1;
    } else {
      const double v = ceil(log(1 - mRansacProb) / log(1 - pow(epsilon, 3)));
      // N == 0 makes this a NaN; the reference converts it all the same, which on x86-64 gives INT_MIN and so one iteration
      nIterations = (v > -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
    }
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mnIterations = 0;
  }

  Matrix4T iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bool bConverge;
    Matrix4T best = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
    if (bConverge) return best;
    Matrix4T I;   // the first overload returns the identity unless it converged (:215)
    SetIdentity(I);
    return I;
  }

  Matrix4T iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    Call c;
    Matrix4T I;
    SetIdentity(I);
    if (!Begin(nIterations, c, bNoMore, vbInliers, nInliers, bConverge)) return I;
    if (c.in.n_hyp > 0) {
      rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
      int rc = rgbl_matcher_acquire(mnDevice, &h);
      if (rc == RGBL_OK) {
        rc = rgbl_sim3_ransac(h, &c.in, &c.out);
        rgbl_matcher_release(h);
      }
      if (rc != RGBL_OK) {
        std::cerr << "[Sim3Solver] " << rgbl_last_error() << std::endl;
        bNoMore = true;
        return I;
      }
    }
    return End(c, bNoMore, vbInliers, nInliers, bConverge);
  }

  Matrix4T find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
  }

  // iterate(nIterations, ...) of several solvers - the candidates of one LoopClosing::DetectCommonRegionsFromBoW pass - in ONE
  // rgbl_sim3_ransac_batch call.  Every vector gets one entry per solver; the samples are drawn solver by solver, in order.
  // With DeviceLocalMaps, the solvers must share one.  false: the call failed (message on stderr), every bNoMore is set.
  static bool SolveBatch(const std::vector<Sim3Solver*>& vpSolvers, int nIterations, std::vector<Matrix4T>& vT12, std::vector<bool>& vbNoMore,
                         std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<bool>& vbConverge) {
    const size_t B = vpSolvers.size();
    std::vector<Call> calls(B);
    std::vector<char> run(B, 0);
    vT12.resize(B); vbNoMore.assign(B, false); vvbInliers.resize(B); vnInliers.assign(B, 0); vbConverge.assign(B, false);
    std::vector<rgbl_sim3_input> in;
    std::vector<size_t> who;
    bool ok = true;
    for (size_t b = 0; b < B; ++b) {
      SetIdentity(vT12[b]);
      bool nm = false, cv = false;
      run[b] = vpSolvers[b]->Begin(nIterations, calls[b], nm, vvbInliers[b], vnInliers[b], cv) ? 1 : 0;
      vbNoMore[b] = nm;
      ok = ok && !vpSolvers[b]->mbRefused;
      if (run[b] && calls[b].in.n_hyp > 0) { in.push_back(calls[b].in); who.push_back(b); }
    }
    std::vector<rgbl_sim3_output> out(in.size());
    for (size_t k = 0; k < in.size(); ++k) out[k] = calls[who[k]].out;
    if (!in.empty()) {
      rgbl_matcher* h = nullptr;
      int rc = rgbl_matcher_acquire(vpSolvers[who[0]]->mnDevice, &h);
      if (rc == RGBL_OK) {
        rc = rgbl_sim3_ransac_batch(h, (int)in.size(), in.data(), out.data());
        rgbl_matcher_release(h);
      }
      if (rc != RGBL_OK) {
        std::cerr << "[Sim3Solver] " << rgbl_last_error() << std::endl;
        vbNoMore.assign(B, true);
        return false;
      }
    }
    for (size_t k = 0; k < in.size(); ++k) calls[who[k]].out = out[k];
    for (size_t b = 0; b < B; ++b) {
      if (!run[b]) continue;
      bool nm = false, cv = false;
      vT12[b] = vpSolvers[b]->End(calls[b], nm, vvbInliers[b], vnInliers[b], cv);
      vbNoMore[b] = nm; vbConverge[b] = cv;
    }
    return ok;
  }

  Matrix4T GetEstimatedTransformation() { return mBestT12; }
  Matrix3T GetEstimatedRotation() { return mBestRotation; }
  Vector3T GetEstimatedTranslation() { return mBestTranslation; }
  float GetEstimatedScale() { return mBestScale; }

  // for tests and diagnostics
  int GetIterations() const { return mnIterations; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetN() const { return N; }
  const std::vector<int32_t>& GetLastSamples() const { return mvLastSamples; }

 private:
  struct SearchBracket {   // as ORBmatcher::SearchLocalPoints: slots erased meanwhile are not handed to other points
    DeviceLocalMap* p;
    explicit SearchBracket(DeviceLocalMap* q) : p(q) { if (p) p->BeginSearch(); }
    ~SearchBracket() { if (p) p->EndSearch(); }
    SearchBracket(const SearchBracket&) = delete;
    SearchBracket& operator=(const SearchBracket&) = delete;
  };
  struct Call {   // one call's arrays; the bracket lasts from before the first SlotOf() until the Call is gone
    rgbl_sim3_input in;
    rgbl_sim3_output out;
    std::vector<int32_t> samples, slot1, slot2;
    std::vector<uint8_t> inlier;
    std::unique_ptr<SearchBracket> bracket;
  };

  static void SetIdentity(Matrix4T& T) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) T(i, j) = i == j ? 1.0f : 0.0f;
  }

  // the head of iterate (:151-186 / :220-259): false = the call is over (N < mRansacMinInliers, or a refused camera)
  bool Begin(int nIterations, Call& c, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    bNoMore = false;
    bConverge = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (mbRefused || N < mRansacMinInliers) {
      bNoMore = true;
      return false;
    }
    const int nRun = std::max(0, std::min(nIterations, mRansacMaxIts - mnIterations));
    c.samples.resize(3 * (size_t)nRun);
    std::vector<size_t> vAvailableIndices;
    for (int k = 0; k < nRun; ++k) {
      vAvailableIndices = mvAllIndices;
      for (short i = 0; i < 3; ++i) {
        int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
        c.samples[3 * (size_t)k + i] = (int32_t)vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    mvLastSamples = c.samples;
    c.in = rgbl_sim3_input();
    c.out = rgbl_sim3_output();
    c.in.n = N;
    if (mpMap) {
      c.bracket.reset(new SearchBracket(mpMap));
      c.slot1.resize((size_t)N); c.slot2.resize((size_t)N);
      std::vector<MapPointT*> vpNew;
      std::vector<std::pair<int, int> > vnNew;
      for (int i = 0; i < N; ++i) {
        c.slot1[i] = mpMap->SlotOf(mvpMapPoints1[i]);
        c.slot2[i] = mpMap->SlotOf(mvpMapPoints2[i]);
        if (c.slot1[i] < 0) { vpNew.push_back(mvpMapPoints1[i]); vnNew.push_back(std::make_pair(1, i)); }
        if (c.slot2[i] < 0) { vpNew.push_back(mvpMapPoints2[i]); vnNew.push_back(std::make_pair(2, i)); }
      }
      bool pooled = true;
      if (!vpNew.empty()) {
        std::vector<int32_t> vnSlots;
        pooled = mpMap->Update(vpNew, &vnSlots);
        for (size_t k = 0; pooled && k < vnNew.size(); ++k) (vnNew[k].first == 1 ? c.slot1 : c.slot2)[vnNew[k].second] = vnSlots[k];
      }
      if (pooled) {
        c.in.pool = mpMap->handle(); c.in.slot1 = c.slot1.data(); c.in.slot2 = c.slot2.data();
        for (int i = 0; i < 9; ++i) { c.in.Rcw1[i] = mRcw1[i]; c.in.Rcw2[i] = mRcw2[i]; }
        for (int i = 0; i < 3; ++i) { c.in.tcw1[i] = mtcw1[i]; c.in.tcw2[i] = mtcw2[i]; }
      }
    }
    if (!c.in.pool) { c.in.x1c = mvX3Dc1.data(); c.in.x2c = mvX3Dc2.data(); }
    c.in.max_err1 = mvnMaxError1.data(); c.in.max_err2 = mvnMaxError2.data();
    for (int i = 0; i < 4; ++i) { c.in.K1[i] = mK1[i]; c.in.K2[i] = mK2[i]; }
    c.in.fix_scale = mbFixScale ? 1 : 0;
    c.in.min_inliers = mRansacMinInliers;
    c.in.best_inliers = mnBestInliers;
    c.in.n_hyp = nRun;
    c.in.samples = c.samples.data();
    c.inlier.assign((size_t)std::max(N, 1), 0);
    c.out.inlier = c.inlier.data();
    c.out.selected = -1;
    c.out.iterations_run = 0;
    return true;
  }

  // the tail of iterate (:192-215 / :265-293) from what the scan left
  Matrix4T End(Call& c, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
    mnIterations += c.out.iterations_run;   // 0 when nothing ran
    if (c.out.selected >= 0) {
      mnBestInliers = c.out.n_inliers;
      mvbBestInliers.assign((size_t)N, false);
      for (int i = 0; i < N; ++i) mvbBestInliers[i] = c.inlier[i] != 0;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) mBestT12(i, j) = c.out.T12[4 * i + j];
      for (int i = 0; i < 3; ++i) {
        mBestTranslation(i) = c.out.t12[i];
        for (int j = 0; j < 3; ++j) mBestRotation(i, j) = c.out.R12[3 * i + j];
      }
      mBestScale = c.out.s12;
      if (c.out.converged) {
        nInliers = c.out.n_inliers;
        for (int i = 0; i < N; i++)
          if (mvbBestInliers[i]) vbInliers[mvnIndices1[i]] = true;
        bConverge = true;
        return mBestT12;
      }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return mBestT12;
  }

  int mnIterations, mnBestInliers;
  bool mbFixScale, mbRefused = false;
  DeviceLocalMap* mpMap;
  int mnDevice;
  int N = 0, mN1 = 0;
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300;
  float mRcw1[9], mtcw1[3], mRcw2[9], mtcw2[3], mK1[4], mK2[4];
  std::vector<MapPointT*> mvpMapPoints1, mvpMapPoints2;
  std::vector<size_t> mvnIndices1, mvAllIndices;
  std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
  std::vector<bool> mvbBestInliers;
  std::vector<int32_t> mvLastSamples;
  Matrix4T mBestT12;
  Matrix3T mBestRotation;
  Vector3T mBestTranslation;
  float mBestScale;
};

}  // namespace rgbl_shim
