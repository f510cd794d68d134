// Sim3Optimizer.h — drop-in for int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1,
// g2o::Sim3& g2oS12, const float th2, const bool bFixScale, Eigen::Matrix<double,7,7>& mAcumHessian, const bool bAllPoints)
// (include/Optimizer.h, src/Optimizer.cc:2115-2381) on the device: one rgbl_optimize_sim3 call, or one
// rgbl_optimize_sim3_batch call for the candidates of a LoopClosing::DetectCommonRegionsFromBoW pass.  INTEGRATION.md shows
// the lines of LoopClosing.cc that change.
//
// Reads pKF->GetRotation(), GetTranslation(), GetMapPointMatches(), mvKeysUn, mvInvLevelSigma2, mpCamera, and of every map
// point isBad(), GetWorldPos() and GetIndexInKeyFrame(pKF2); clears the entries of vpMatches1 the
// reference clears, writes g2oS12 (not when the reference returns at :2349), zeroes mAcumHessian where the reference does
// (:2356: not before the early return) and returns the reference's value.  The gathering stays on the host, as the
// reference's set-up loop does; the arrays go up with the call.
//
// A match that is not observed in pKF2 gets level 0, as in the reference as compiled: :2280 hands mnTrackScaleLevel to
// cv::KeyPoint(Point2f, float size, ...) as the SIZE, so kpUn2.octave stays 0 and :2291 reads mvInvLevelSigma2[0].  The member
// itself is not read here (Frame.cc:668 sets it to -1 outside the frustum, and the constructors leave it uninitialised).
//
// Sim3T is g2o::Sim3 or anything with its accessors: rotation() whose coeffs are x(), y(), z(), w() (read and written),
// translation()(i), scale(), all three also as lvalues.  HessianT needs operator()(row, col).
//
// Pinhole cameras only: a key frame whose camera is not a Pinhole (GeometricCamera::CAM_PINHOLE) is refused with a message,
// returns -1 and leaves everything untouched.
#pragma once
#include <string.h>

#include <iostream>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace rgbl_shim {

// the arrays of one call; they live until the call has returned
template <class KeyFrameT>
struct Sim3OptGather {
  typedef typename std::remove_pointer<typename std::decay<decltype(std::declval<KeyFrameT>().GetMapPointMatches()[0])>::type>::type MapPointT;
  std::vector<int32_t> mp1, match, i2, lvl2, oct1, oct2;
  std::vector<uint8_t> bad, cleared;
  std::vector<float> pos, xy1, xy2;
  rgbl_sim3_opt_input in;
  rgbl_sim3_opt_output out;
  bool refused = false;

  template <class Sim3T>
  Sim3OptGather(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatches1, const Sim3T& g2oS12, float th2, bool bFixScale,
                bool bAllPoints) {
    memset(&in, 0, sizeof(in));
    memset(&out, 0, sizeof(out));
    if (pKF1->mpCamera->GetType() != 0u || pKF2->mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) {
      std::cerr << "[OptimizeSim3] only Pinhole cameras are covered by the device path" << std::endl;
      refused = true;
      return;
    }
    const int N = (int)vpMatches1.size();
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    mp1.assign((size_t)N, -1); match.assign((size_t)N, -1); i2.assign((size_t)N, -1); lvl2.assign((size_t)N, 0);
    auto add = [&](MapPointT* p) {
      const auto P = p->GetWorldPos();
      for (int k = 0; k < 3; ++k) pos.push_back(P(k));
      bad.push_back(p->isBad() ? 1 : 0);
      return (int32_t)bad.size() - 1;
    };
    for (int i = 0; i < N; ++i) {
      MapPointT* pMP2 = vpMatches1[(size_t)i];
      if (!pMP2) continue;
      match[(size_t)i] = add(pMP2);
      i2[(size_t)i] = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
      if (i < (int)vpMapPoints1.size() && vpMapPoints1[(size_t)i]) mp1[(size_t)i] = add(vpMapPoints1[(size_t)i]);
    }
    auto keys = [](KeyFrameT* kf, std::vector<float>& xy, std::vector<int32_t>& oct) {
      for (const auto& kp : kf->mvKeysUn) { xy.push_back(kp.pt.x); xy.push_back(kp.pt.y); oct.push_back(kp.octave); }
    };
    keys(pKF1, xy1, oct1);
    keys(pKF2, xy2, oct2);
    if ((int)oct1.size() < N) { xy1.resize(2 * (size_t)N, 0.0f); oct1.resize((size_t)N, 0); }   // a match list longer than the key frame
    const auto R1 = pKF1->GetRotation(), R2 = pKF2->GetRotation();
    const auto t1 = pKF1->GetTranslation(), t2 = pKF2->GetTranslation();
    for (int r = 0; r < 3; ++r) {
      in.tcw1[r] = t1(r); in.tcw2[r] = t2(r);
      for (int c = 0; c < 3; ++c) { in.Rcw1[3 * r + c] = R1(r, c); in.Rcw2[3 * r + c] = R2(r, c); }
    }
    for (int k = 0; k < 4; ++k) { in.K1[k] = pKF1->mpCamera->getParameter(k); in.K2[k] = pKF2->mpCamera->getParameter(k); }
    cleared.assign((size_t)N, 0);
    in.n = N; in.mp1_index = mp1.data(); in.match_index = match.data(); in.i2 = i2.data(); in.track_level2 = lvl2.data();
    in.n_points = (int)bad.size(); in.bad = bad.data(); in.world_pos = pos.data();
    in.kp1_xy = xy1.data(); in.kp1_octave = oct1.data();
    in.n2 = (int)oct2.size(); in.kp2_xy = xy2.data(); in.kp2_octave = oct2.data();
    in.inv_level_sigma2_1 = pKF1->mvInvLevelSigma2.data(); in.n_levels1 = (int)pKF1->mvInvLevelSigma2.size();
    in.inv_level_sigma2_2 = pKF2->mvInvLevelSigma2.data(); in.n_levels2 = (int)pKF2->mvInvLevelSigma2.size();
    in.q[0] = g2oS12.rotation().x(); in.q[1] = g2oS12.rotation().y(); in.q[2] = g2oS12.rotation().z(); in.q[3] = g2oS12.rotation().w();
    for (int k = 0; k < 3; ++k) in.t[k] = g2oS12.translation()(k);
    in.s = g2oS12.scale();
    in.th2 = th2; in.fix_scale = bFixScale ? 1 : 0; in.all_points = bAllPoints ? 1 : 0;
    out.cleared = cleared.data();
  }

  // what the reference leaves in its arguments (:2323, :2349, :2356, :2369, :2378)
  template <class Sim3T, class HessianT>
  int Finish(std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, HessianT& mAcumHessian) {
    for (size_t i = 0; i < cleared.size(); ++i)
      if (cleared[i]) vpMatches1[i] = static_cast<MapPointT*>(nullptr);
    if (out.diag.rounds < 2) return 0;   // :2349: g2oS12 and mAcumHessian are not written
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) mAcumHessian(r, c) = 0.0;
    g2oS12.rotation().x() = out.q[0]; g2oS12.rotation().y() = out.q[1]; g2oS12.rotation().z() = out.q[2]; g2oS12.rotation().w() = out.q[3];
    for (int k = 0; k < 3; ++k) g2oS12.translation()(k) = out.t[k];
    g2oS12.scale() = out.s;
    return out.result;
  }
};

template <class KeyFrameT, class MapPointT, class Sim3T, class HessianT>
int OptimizeSim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale,
                 HessianT& mAcumHessian, const bool bAllPoints = false, int device = 0) {
  Sim3OptGather<KeyFrameT> g(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, bAllPoints);
  if (g.refused) return -1;
  rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
  int rc = rgbl_matcher_acquire(device, &h);
  if (rc == RGBL_OK) {
    rc = rgbl_optimize_sim3(h, &g.in, &g.out);
    rgbl_matcher_release(h);
  }
  if (rc != RGBL_OK) {
    std::cerr << "[OptimizeSim3] " << rgbl_last_error() << std::endl;
    return -1;
  }
  return g.Finish(vpMatches1, g2oS12, mAcumHessian);
}

// The candidates of one pass in ONE rgbl_optimize_sim3_batch call: candidate b is (pKF1, vpKF2[b], *vvpMatches1[b], vS12[b],
// vHessian[b]); vnResult[b] gets what OptimizeSim3 would return.  false: a camera was refused or the call failed (message on
// stderr); nothing is written then.
template <class KeyFrameT, class MapPointT, class Sim3T, class HessianT>
bool OptimizeSim3Batch(KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpKF2, const std::vector<std::vector<MapPointT*>*>& vvpMatches1,
                       std::vector<Sim3T>& vS12, const float th2, const bool bFixScale, std::vector<HessianT>& vHessian, std::vector<int>& vnResult,
                       const bool bAllPoints = false, int device = 0) {
  const size_t B = vpKF2.size();
  std::vector<Sim3OptGather<KeyFrameT>*> g(B, nullptr);
  struct Owner {
    std::vector<Sim3OptGather<KeyFrameT>*>& v;
    ~Owner() { for (auto* p : v) delete p; }
  } owner{g};
  std::vector<rgbl_sim3_opt_input> in(B);
  std::vector<rgbl_sim3_opt_output> out(B);
  for (size_t b = 0; b < B; ++b) {
    g[b] = new Sim3OptGather<KeyFrameT>(pKF1, vpKF2[b], *vvpMatches1[b], vS12[b], th2, bFixScale, bAllPoints);
    if (g[b]->refused) return false;
    in[b] = g[b]->in;
    out[b] = g[b]->out;
  }
  vnResult.assign(B, 0);
  if (B == 0) return true;
  rgbl_matcher* h = nullptr;
  int rc = rgbl_matcher_acquire(device, &h);
  if (rc == RGBL_OK) {
    rc = rgbl_optimize_sim3_batch(h, (int)B, in.data(), out.data());
    rgbl_matcher_release(h);
  }
  if (rc != RGBL_OK) {
    std::cerr << "[OptimizeSim3] " << rgbl_last_error() << std::endl;
    return false;
  }
  for (size_t b = 0; b < B; ++b) {
    g[b]->out = out[b];
    vnResult[b] = g[b]->Finish(*vvpMatches1[b], vS12[b], vHessian[b]);
  }
  return true;
}

}  // namespace rgbl_shim
