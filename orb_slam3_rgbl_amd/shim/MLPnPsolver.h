// MLPnPsolver.h — drop-in for ORB_SLAM3::MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp) with the RANSAC on the device: a
// call of iterate is ONE rgbl_mlpnp_ransac call that evaluates every hypothesis the call may run.  INTEGRATION.md shows the
// lines of Tracking::Relocalization that change.
//
//   typedef rgbl_shim::MLPnPsolver<Frame, MapPoint> MLPnPsolver;
//
// DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.h) must be declared before this header is included.  Tout is any 4 x 4
// with operator()(row, col) (Eigen::Matrix4f).
//
// What stays on the host, as in the reference: the constructor's bookkeeping (:55-97: isBad, the features beyond mvKeysUn,
// mvKeyPointIndices), SetRansacParameters (:225-260, with its pow(epsilon, 3) although the minimal set is 6), the
// N < mRansacMinInliers exit (:106-110) and the drawing of the samples with DUtils::Random::RandomInt and the swap-and-pop of
// vAvailableIndices (:128-140).  mnIterations, mnBestInliers, mvbBestInliers and mBestTcw persist across calls.
//
// Deviations from the reference:
//   - a call draws the six-sets of ALL the iterations it may run - max(mRansacMaxIts - mnIterations, nIterations), the `||` of
//     :115 - before it knows where the scan stops.  After a call that succeeded early the process-wide rand() stream is
//     therefore further along than the reference's; the call's own result is not affected;
//   - mBestTcw is the identity before any hypothesis was held (uninitialised in the reference; never handed out then);
//   - the arithmetic inside computePose is this project's restatement (csrc/mlpnp_math.h lists what is pinned).
// Refine (:295-353) is what the reference COMPILES to: it returns the current hypothesis (csrc/mlpnp_math.h, ml_scan).
//
// Pinhole cameras only, minimal sets of six only: a frame whose camera is not a Pinhole (GeometricCamera::CAM_PINHOLE), or a
// SetRansacParameters with minSet != 6, is refused with a message; every iterate then returns false with bNoMore = true.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <iostream>
#include <vector>

#include "rgbl_frontend.h"

namespace rgbl_shim {

template <class FrameT, class MapPointT>
class MLPnPsolver {
 public:
  MLPnPsolver(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches, int device = 0)
      : mnIterations(0), mnBestInliers(0), N(0), mnDevice(device), mbRefused(false) {
    for (int i = 0; i < 16; ++i) mBestTcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    if (F.mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) {
      std::cerr << "rgbl_shim::MLPnPsolver: the camera is not a Pinhole; this solver stays on the reference's path" << std::endl;
      mbRefused = true;
    }
    for (int i = 0; i < 4; ++i) mK[i] = F.mpCamera->getParameter(i);
    const size_t n = vpMapPointMatches.size();
    mvMpIndex.assign(n, -1);
    mvXY.assign(2 * n, 0.0f);
    mvOctave.assign(n, 0);
    mvLevelSigma2.assign(F.mvLevelSigma2.begin(), F.mvLevelSigma2.end());
    for (size_t i = 0; i < n; ++i) {
      if (i < F.mvKeysUn.size()) {
        mvXY[2 * i] = F.mvKeysUn[i].pt.x; mvXY[2 * i + 1] = F.mvKeysUn[i].pt.y;
        mvOctave[i] = F.mvKeysUn[i].octave;
      }
      MapPointT* pMP = vpMapPointMatches[i];
      if (!pMP || pMP->isBad() || i >= F.mvKeysUn.size()) continue;   // :69-71
      const auto pos = pMP->GetWorldPos();
      mvMpIndex[i] = N++;
      mvKeyPointIndices.push_back(i);
      for (int c = 0; c < 3; ++c) mvWorldPos.push_back(pos(c));
    }
    SetRansacParameters();
  }

  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    mRansacProb = probability; mRansacMinInliers = minInliers; mRansacMaxIts = maxIterations; mRansacEpsilon = epsilon; mRansacMinSet = minSet;
    if (minSet != 6) {
      std::cerr << "rgbl_shim::MLPnPsolver: minimal sets of " << minSet << " have no device form" << std::endl;
      mbRefused = true;
    }
    int nMinInliers = N * mRansacEpsilon;
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) nIterations = 1;
    else if (!(pow(mRansacEpsilon, 3) < 1.0)) nIterations = mRansacMaxIts;   // N < mRansacMinInliers: the reference converts a NaN here; iterate leaves before it matters
    else nIterations = (int)ceil(log(1 - mRansacProb) / log(1 - pow(mRansacEpsilon, 3)));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mRansacTh2 = th2;
  }

  template <class Matrix4T>
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Matrix4T& Tout) {
    Call c;
    if (!Prepare(nIterations, c)) return Finish(c, false, bNoMore, vbInliers, nInliers, Tout);
    rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
    int rc = rgbl_matcher_acquire(mnDevice, &h);
    if (rc == RGBL_OK) {
      rc = rgbl_mlpnp_ransac(h, &c.in, &c.out);
      rgbl_matcher_release(h);
    }
    if (rc != RGBL_OK) std::cerr << "rgbl_shim::MLPnPsolver: " << rgbl_last_error() << std::endl;
    return Finish(c, rc == RGBL_OK, bNoMore, vbInliers, nInliers, Tout);
  }

  // One iterate(nIterations, ...) of every solver of one pass of the loop at Tracking.cc:3703 in ONE rgbl_mlpnp_ransac_batch
  // call.  Every vector gets one entry per solver (vbNoMore, vbFound: 0 / 1); the samples are drawn solver by solver, in order.
  // The solvers of a batch must have been constructed for the same device: a mixed batch is refused with a message before
  // anything is drawn - false is returned, and every solver reports bNoMore without having run.  False also when the call fails.
  template <class Matrix4T>
  static bool IterateBatch(const std::vector<MLPnPsolver*>& vpSolvers, int nIterations, std::vector<char>& vbNoMore,
                           std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers, std::vector<Matrix4T>& vTout,
                           std::vector<char>& vbFound) {
    const size_t B = vpSolvers.size();
    std::vector<Call> calls(B);
    std::vector<rgbl_mlpnp_input> in;
    std::vector<rgbl_mlpnp_output> out;
    std::vector<size_t> who;
    for (size_t b = 1; b < B; ++b)
      if (vpSolvers[b]->mnDevice != vpSolvers[0]->mnDevice) {
        std::cerr << "rgbl_shim::MLPnPsolver::IterateBatch: solver " << b << " is on device " << vpSolvers[b]->mnDevice << ", solver 0 on "
                  << vpSolvers[0]->mnDevice << "; the solvers of one batch share a device" << std::endl;
        vbNoMore.assign(B, 1); vvbInliers.assign(B, std::vector<bool>()); vnInliers.assign(B, 0); vbFound.assign(B, 0);
        vTout.assign(B, Matrix4T());
        for (size_t k = 0; k < B; ++k)
          for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) vTout[k](i, j) = i == j ? 1.0f : 0.0f;
        return false;
      }
    for (size_t b = 0; b < B; ++b)
      if (vpSolvers[b]->Prepare(nIterations, calls[b])) { who.push_back(b); in.push_back(calls[b].in); out.push_back(calls[b].out); }
    bool ok = true;
    if (!who.empty()) {
      rgbl_matcher* h = nullptr;
      int rc = rgbl_matcher_acquire(vpSolvers[who[0]]->mnDevice, &h);
      if (rc == RGBL_OK) {
        rc = rgbl_mlpnp_ransac_batch(h, (int)in.size(), in.data(), out.data());
        rgbl_matcher_release(h);
      }
      if (rc != RGBL_OK) std::cerr << "rgbl_shim::MLPnPsolver: " << rgbl_last_error() << std::endl;
      ok = rc == RGBL_OK;
    }
    for (size_t k = 0; k < who.size(); ++k) calls[who[k]].out = out[k];
    vbNoMore.assign(B, 0); vvbInliers.assign(B, std::vector<bool>()); vnInliers.assign(B, 0); vTout.assign(B, Matrix4T()); vbFound.assign(B, 0);
    for (size_t b = 0; b < B; ++b) {
      bool no_more = false;
      vbFound[b] = vpSolvers[b]->Finish(calls[b], ok, no_more, vvbInliers[b], vnInliers[b], vTout[b]) ? 1 : 0;
      vbNoMore[b] = no_more ? 1 : 0;
    }
    return ok;
  }

  int GetIterations() const { return mnIterations; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetMinInliers() const { return mRansacMinInliers; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetN() const { return N; }
  const float* GetBestTcw() const { return mBestTcw; }   // mBestTcw, row-major
  const std::vector<int32_t>& LastSamples() const { return mvLastSamples; }   // the sets of the last call, n_hyp x 6, as drawn

 private:
  struct Call {
    rgbl_mlpnp_input in;
    rgbl_mlpnp_output out;
    std::vector<uint8_t> inlier, best;
    bool launched = false;
  };
  // fills the call; false: nothing to run (refused, N < mRansacMinInliers, no iteration left)
  bool Prepare(int nIterations, Call& c) {
    memset(&c.in, 0, sizeof(c.in));
    memset(&c.out, 0, sizeof(c.out));
    if (mbRefused || N < mRansacMinInliers) return false;
    const int n_hyp = std::max(mRansacMaxIts - mnIterations, nIterations);   // `||` (:115)
    if (n_hyp <= 0) return false;
    mvLastSamples.assign(6 * (size_t)n_hyp, 0);
    for (int k = 0; k < n_hyp; ++k) {   // :120-140
      std::vector<size_t> vAvailableIndices((size_t)N);
      for (int i = 0; i < N; ++i) vAvailableIndices[i] = (size_t)i;
      for (short i = 0; i < 6; ++i) {
        const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
        mvLastSamples[6 * (size_t)k + i] = (int32_t)vAvailableIndices[randi];
        vAvailableIndices[randi] = vAvailableIndices.back();
        vAvailableIndices.pop_back();
      }
    }
    rgbl_mlpnp_input& I = c.in;
    I.n = (int)mvMpIndex.size(); I.mp_index = mvMpIndex.data(); I.n_points = N; I.world_pos = mvWorldPos.data();
    I.kp_xy = mvXY.data(); I.kp_octave = mvOctave.data();
    memcpy(I.K, mK, sizeof(mK));
    I.level_sigma2 = mvLevelSigma2.data(); I.n_levels = (int)mvLevelSigma2.size(); I.th2 = mRansacTh2;
    I.min_inliers = mRansacMinInliers; I.best_inliers = mnBestInliers; I.best_mask = mnBestInliers > 0 ? mvbBestInliers.data() : nullptr;
    memcpy(I.best_Tcw, mBestTcw, sizeof(mBestTcw));
    I.n_hyp = n_hyp; I.samples = mvLastSamples.data();
    c.inlier.assign(mvMpIndex.size(), 0);
    c.best.assign((size_t)N, 0);
    c.out.inlier = c.inlier.data(); c.out.best_mask = c.best.data();
    c.launched = true;
    return true;
  }
  template <class Matrix4T>
  bool Finish(Call& c, bool ok, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Matrix4T& Tout) {
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) Tout(i, j) = i == j ? 1.0f : 0.0f;   // :101-104
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (mbRefused || N < mRansacMinInliers || (c.launched && !ok)) { bNoMore = true; return false; }
    if (!c.launched) {   // no iteration left: the tail of :205-222
      if (mnIterations < mRansacMaxIts) return false;
      bNoMore = true;
      if (mnBestInliers < mRansacMinInliers) return false;
      nInliers = mnBestInliers;
      vbInliers.assign(mvMpIndex.size(), false);
      for (int i = 0; i < N; ++i) if (mvbBestInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
      for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Tout(i, j) = mBestTcw[4 * i + j];
      return true;
    }
    const rgbl_mlpnp_output& O = c.out;
    mnIterations += O.iterations_run;
    mnBestInliers = O.best_inliers;
    if (O.best_inliers > 0) mvbBestInliers = c.best;
    memcpy(mBestTcw, O.best_Tcw, sizeof(mBestTcw));
    bNoMore = O.no_more != 0;
    if (!O.found) return false;
    nInliers = O.n_inliers;
    vbInliers.assign(mvMpIndex.size(), false);
    for (size_t i = 0; i < c.inlier.size(); ++i) vbInliers[i] = c.inlier[i] != 0;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) Tout(i, j) = O.Tcw[4 * i + j];
    return true;
  }

  std::vector<int32_t> mvMpIndex, mvOctave, mvLastSamples;
  std::vector<float> mvXY, mvWorldPos, mvLevelSigma2;
  std::vector<size_t> mvKeyPointIndices;
  std::vector<uint8_t> mvbBestInliers;
  float mK[4], mBestTcw[16], mRansacTh2;
  int mnIterations, mnBestInliers, N;
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts, mRansacMinSet;
  float mRansacEpsilon;
  int mnDevice;
  bool mbRefused;
};

}  // namespace rgbl_shim
