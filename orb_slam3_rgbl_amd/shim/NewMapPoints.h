// NewMapPoints.h — drop-in for the neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:434-693) on the
// device: one rgbl_create_new_map_points call instead of one SearchForTriangulation per neighbour with the per-match block on
// the host between them.  INTEGRATION.md shows the lines it replaces; the caller keeps :390-432 and walks the returned list
// through :694-709 (new MapPoint, AddObservation, AddMapPoint, Atlas).
//
// Single-camera pinhole key frames (mpCamera2 == nullptr, NLeft == -1); a rig key frame is refused (false, nothing returned).
// Key frames are flattened the way ORBmatcher::SearchForTriangulation flattens them - GetMapPoint(), GetPose() and
// GetCameraCenter() take the key frame's own mutexes, as the reference's loop does - and a key frame with a resident copy
// (KeyFrame::mpDeviceFrame, LocalMap.h) uploads neither descriptors nor key points.
#pragma once
#include <iostream>
#include <vector>

#include "ORBmatcher.h"

namespace rgbl_shim {

template <class KeyFrameT>
struct NewMapPoint {
  KeyFrameT* pKF2;   // the neighbour
  int idx1, idx2;    // mpCurrentKeyFrame's feature, pKF2's feature
  float x3D[3];
  bool stereo;       // bPointStereo (:581, :695)
};

// ORBmatcher's flattening and the handle of the caller's matcher: only that matcher owns a handle, nothing here acquires one
struct NewPointsAccess {
  typedef ORB_SLAM3::ORBmatcher::Flat Flat;
  template <class KeyFrameT> static void Flatten(KeyFrameT* p, Flat& f) { ORB_SLAM3::ORBmatcher::Flatten(p, f); }
  static rgbl_matcher* HandleOf(ORB_SLAM3::ORBmatcher& m) { return m.mpHandle; }
};

// what rgbl_new_points_keyframe points into: one key frame's flattened arrays, plain host memory
struct NewPointsFlat {
  NewPointsAccess::Flat flat;
  std::vector<float> raw;
  rgbl_new_points_keyframe kf{};
  template <class KeyFrameT>
  void Fill(KeyFrameT* p) {
    flat = NewPointsAccess::Flat();   // Flatten appends to the FeatureVector arrays
    NewPointsAccess::Flatten(p, flat);
    const int n = p->N;
    raw.resize(2 * (size_t)n);
    for (int i = 0; i < n; ++i) { raw[2 * i] = p->mvKeys[i].pt.x; raw[2 * i + 1] = p->mvKeys[i].pt.y; }
    kf.view = flat.view;
    kf.depth = p->mvDepth.data();
    kf.kp_xy_raw = raw.data();
    const auto Tcw = p->GetPose();
    const auto R = Tcw.rotationMatrix();
    const auto t = Tcw.translation();
    const auto Ow = p->GetCameraCenter();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) kf.Tcw[4 * r + c] = R(r, c);
      kf.Tcw[4 * r + 3] = t(r);
      kf.Ow[r] = Ow(r);
    }
    for (int i = 0; i < 4; ++i) kf.K[i] = p->mpCamera->getParameter(i);
    kf.mb = p->mb;
    kf.mbf = p->mbf;
    kf.scale_factors = p->mvScaleFactors.data();
    kf.level_sigma2 = p->mvLevelSigma2.data();
  }
};

// F12 and the epipole of one neighbour as ORBmatcher::SearchForTriangulation computes them (ORBmatcher.cc:913-931)
template <class KeyFrameT>
void TriangulationParamsOf(KeyFrameT* pKF1, KeyFrameT* pKF2, bool bCoarse, rgbl_triangulation_params& prm) {
  auto T12 = pKF1->GetPose() * pKF2->GetPoseInverse();
  auto R = T12.rotationMatrix();
  auto t = T12.translation();
  auto C2 = pKF2->GetPose() * pKF1->GetCameraCenter();
  auto ep = pKF2->mpCamera->project(C2);
  float R12[9], t12[3], K1[4], K2[4];
  for (int i = 0; i < 3; ++i) {
    t12[i] = t(i);
    for (int j = 0; j < 3; ++j) R12[3 * i + j] = R(i, j);
  }
  for (int i = 0; i < 4; ++i) {
    K1[i] = pKF1->mpCamera->getParameter(i);
    K2[i] = pKF2->mpCamera->getParameter(i);
  }
  rgbl_fundamental(K1, K2, R12, t12, prm.F12);
  prm.epipole[0] = ep(0);
  prm.epipole[1] = ep(1);
  prm.scale_factors2 = pKF2->mvScaleFactors.data();
  prm.level_sigma2_2 = pKF2->mvLevelSigma2.data();
  prm.n_levels = (int)pKF2->mvScaleFactors.size();
  prm.only_stereo = 0;
  prm.coarse = bCoarse;
  prm.check_orientation = 0;   // LocalMapping.cc:412
}

// vpNeighKFs in the order of the reference's loop; pvSkip (nullable): the caller's monocular median-depth test (:455-459), one
// entry per neighbour.  vNew: the accepted matches in the reference's order - neighbour after neighbour, ascending idx1.
// pvMatches (nullable): what SearchForTriangulation returned per neighbour, -1 for one left out.
template <class KeyFrameT>
bool CreateNewMapPoints(ORB_SLAM3::ORBmatcher& matcher, KeyFrameT* pKF, const std::vector<KeyFrameT*>& vpNeighKFs, bool bMonocular,
                        bool bInertial, bool bCoarse, bool bFarPoints, float thFarPoints, const std::vector<unsigned char>* pvSkip,
                        std::vector<NewMapPoint<KeyFrameT> >& vNew, std::vector<int>* pvMatches = nullptr) {
  vNew.clear();
  rgbl_matcher* h = NewPointsAccess::HandleOf(matcher);
  if (!h) return false;
  const int nn = (int)vpNeighKFs.size();
  bool rig = pKF->mpCamera2 || pKF->NLeft != -1;
  for (KeyFrameT* p : vpNeighKFs) rig = rig || p->mpCamera2 || p->NLeft != -1;
  if (rig) {
    std::cerr << "[CreateNewMapPoints] fisheye stereo rigs (mpCamera2) are not covered by the device path" << std::endl;
    return false;
  }
  NewPointsFlat f1;
  f1.Fill(pKF);
  std::vector<NewPointsFlat> f2((size_t)nn);
  std::vector<rgbl_new_points_keyframe> k2((size_t)nn);
  std::vector<rgbl_triangulation_params> tp((size_t)nn);
  for (int i = 0; i < nn; ++i) {
    f2[i].Fill(vpNeighKFs[i]);
    k2[i] = f2[i].kf;
    TriangulationParamsOf(pKF, vpNeighKFs[i], bCoarse, tp[i]);
  }
  rgbl_new_points_params prm;
  prm.n_levels = (int)pKF->mvScaleFactors.size();
  prm.ratio_factor = 1.5f * pKF->mfScaleFactor;   // :428
  prm.far_points = bFarPoints;
  prm.th_far_points = thFarPoints;
  prm.inertial = bInertial;
  prm.monocular = bMonocular;
  prm.report_rejected = 0;
  std::vector<rgbl_new_point> rec((size_t)(f1.kf.view.n > 0 ? f1.kf.view.n : 1));
  std::vector<int32_t> per((size_t)(nn > 0 ? nn : 1), 0);
  int n_out = 0;
  if (rgbl_create_new_map_points(h, &f1.kf, nn, k2.data(), tp.data(), pvSkip ? pvSkip->data() : nullptr, &prm, rec.data(), f1.kf.view.n,
                                 &n_out, per.data(), nullptr) != RGBL_OK) {
    std::cerr << "[CreateNewMapPoints] " << rgbl_last_error() << std::endl;
    return false;
  }
  vNew.reserve((size_t)n_out);
  for (int i = 0; i < n_out; ++i) {
    NewMapPoint<KeyFrameT> p;
    p.pKF2 = vpNeighKFs[rec[i].neighbour];
    p.idx1 = rec[i].idx1; p.idx2 = rec[i].idx2;
    for (int c = 0; c < 3; ++c) p.x3D[c] = rec[i].x3D[c];
    p.stereo = rec[i].status != 1;
    vNew.push_back(p);
  }
  if (pvMatches) pvMatches->assign(per.begin(), per.begin() + nn);
  return true;
}

}  // namespace rgbl_shim
