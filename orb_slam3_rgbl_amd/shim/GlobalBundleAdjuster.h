// GlobalBundleAdjuster.h — drop-ins for void Optimizer::BundleAdjustment(const vector<KeyFrame*>& vpKFs, const vector<MapPoint*>&
// vpMP, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) and Optimizer::GlobalBundleAdjustemnt
// (include/Optimizer.h, src/Optimizer.cc:52-390) on the device: the vertex and edge loops (:116-275) on the host in the
// reference's order, ONE rgbl_bundle_adjustment call for :279-280, then the write-back :285-389.  INTEGRATION.md shows the lines
// of LoopClosing.cc and Tracking.cc that change.
//
// Reads of a key frame mnId, isBad(), GetMap(), GetPose(), mvKeysUn, mvuRight, mvInvLevelSigma2, mpCamera, mpCamera2, fx, fy,
// cx, cy, mbf; of a map point mnId, isBad(), GetObservations(), GetWorldPos(); of the map GetInitKFid() and GetOriginKF().
// Writes: with nLoopKF == pMap->GetOriginKF()->mnId (the initialisation, Tracking.cc:2614) SetPose of every key frame that is
// not bad, SetWorldPos and UpdateNormalAndDepth of every point that is not bad and was included; otherwise (loop closing,
// LoopClosing.cc:2284) mTcwGBA and mnBAGlobalForKF of those key frames, mPosGBA and mnBAGlobalForKF of those points.
//
// The order is the reference's.  Cameras: vpKFs without the bad ones, in vector order; the one whose mnId is the map's
// GetInitKFid() is fixed (:125).  Points: vpMP without the bad ones.  Edges: point-major, within a point in the order of its
// observations map (std::map<KeyFrame*, ...>: by pointer), skipping a key frame that is bad, whose mnId is beyond the largest
// of vpKFs (:154) or that has no vertex (:156); a monocular edge reads K from mpCamera->getParameter(0 .. 3), a stereo edge from
// fx, fy, cx, cy and mbf.  nEdges (:158) counts an observation BEFORE its left index is looked at, so a point seen only through
// left index -1 stays included, without an edge: it is written back as it came.  bRobust and nIterations go to the call as they
// are, pbStopFlag as the byte g2o polls.
//
// NOT restated: the block :306-363.  It only fills locals that nobody reads (numMonoBadPoints, vpMonoMPsOpt, ...), and its
// stereo loop indexes vpEdgeKFMono with a stereo edge's index.  :299 builds the pose as Sophus::SE3d and casts it; here both
// branches hand the estimate's quaternion and translation, cast to float, to the SE3f constructor as :295 does.
//
// Returns true when the reference's work was done here.  false, with NOTHING written: a key frame with a second camera (the rig
// edge :229-261), a camera that is not a Pinhole, a key frame whose monocular and stereo intrinsics differ, a limit of the C ABI
// exceeded (1 024 active key frames, 2^18 points, 2^20 edges), or a failed call (message on stderr) - the caller then runs
// Optimizer::BundleAdjustment.
#pragma once
#include <string.h>

#include <iostream>
#include <map>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace rgbl_shim {

template <class KeyFrameT, class MapPointT>
bool BundleAdjustment(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, int nIterations = 5, bool* pbStopFlag = nullptr,
                      const unsigned long nLoopKF = 0, const bool bRobust = true, int device = 0) {
  if (vpKFs.empty()) return true;
  auto* pMap = vpKFs[0]->GetMap();   // :66
  // :116-129
  std::vector<KeyFrameT*> cams;
  std::map<unsigned long, int> vertex;   // optimizer.vertex(pKF->mnId)
  unsigned long maxKFid = 0;
  for (KeyFrameT* pKF : vpKFs) {
    if (pKF->isBad()) continue;
    vertex[pKF->mnId] = (int)cams.size();
    cams.push_back(pKF);
    if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
  }
  const int nC = (int)cams.size();
  std::vector<uint8_t> fixed((size_t)nC, 0);
  std::vector<float> q(4 * (size_t)nC), t(3 * (size_t)nC), K(4 * (size_t)nC), bf((size_t)nC);
  for (int c = 0; c < nC; ++c) {
    KeyFrameT* k = cams[(size_t)c];
    if (k->mpCamera2) { std::cerr << "[BundleAdjustment] two-camera key frames are not covered by the device path" << std::endl; return false; }
    if (k->mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) { std::cerr << "[BundleAdjustment] only Pinhole cameras are covered by the device path" << std::endl; return false; }
    const float Kc[4] = {k->fx, k->fy, k->cx, k->cy};
    for (int i = 0; i < 4; ++i) {
      if (k->mpCamera->getParameter(i) != Kc[i]) { std::cerr << "[BundleAdjustment] a key frame's camera and its fx, fy, cx, cy differ" << std::endl; return false; }
      K[4 * (size_t)c + i] = Kc[i];
    }
    bf[(size_t)c] = k->mbf;
    const auto Tcw = k->GetPose();
    const auto uq = Tcw.unit_quaternion();
    const auto tr = Tcw.translation();
    q[4 * (size_t)c] = uq.x(); q[4 * (size_t)c + 1] = uq.y(); q[4 * (size_t)c + 2] = uq.z(); q[4 * (size_t)c + 3] = uq.w();
    for (int i = 0; i < 3; ++i) t[3 * (size_t)c + i] = tr(i);
    fixed[(size_t)c] = k->mnId == pMap->GetInitKFid() ? 1 : 0;   // :125
  }
  // :135-275
  std::vector<MapPointT*> pts;
  std::vector<uint8_t> included;   // !vbNotIncludedMP of the points that are not bad
  std::vector<float> pos, obs, info;
  std::vector<int32_t> edge_point, edge_cam;
  for (MapPointT* pMP : vpMP) {
    if (pMP->isBad()) continue;
    const int p = (int)pts.size();
    pts.push_back(pMP);
    const auto X = pMP->GetWorldPos();
    for (int i = 0; i < 3; ++i) pos.push_back(X(i));
    const auto observations = pMP->GetObservations();
    int nEdges = 0;
    for (const auto& ob : observations) {
      KeyFrameT* pKF = ob.first;
      if (pKF->isBad() || pKF->mnId > maxKFid) continue;
      const auto it = vertex.find(pKF->mnId);
      if (it == vertex.end()) continue;
      ++nEdges;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex == -1) continue;
      const float ur = pKF->mvuRight[(size_t)leftIndex];
      if (!(ur < 0) && !(ur >= 0)) continue;   // :162 / :192: neither branch takes a NaN
      const auto& kpUn = pKF->mvKeysUn[(size_t)leftIndex];
      edge_point.push_back(p); edge_cam.push_back(it->second);
      obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(ur < 0 ? -1.0f : ur);
      info.push_back(pKF->mvInvLevelSigma2[(size_t)kpUn.octave]);
    }
    included.push_back(nEdges == 0 ? 0 : 1);   // :266-274
  }
  const int nP = (int)pts.size(), nE = (int)edge_point.size();

  rgbl_ba_input in;
  rgbl_ba_output out;
  memset(&in, 0, sizeof(in));
  memset(&out, 0, sizeof(out));
  in.n_cams = nC; in.cam_is_fixed = fixed.data();
  in.cam_q = q.data(); in.cam_t = t.data(); in.cam_K = K.data(); in.cam_bf = bf.data();
  in.n_points = nP; in.world_pos = pos.data();
  in.n_edges = nE; in.edge_point = edge_point.data(); in.edge_cam = edge_cam.data(); in.edge_obs = obs.data(); in.edge_inv_sigma2 = info.data();
  in.robust = bRobust ? 1 : 0;        // :177, :209
  in.max_iterations = nIterations;    // :280
  static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
  in.stop_byte = reinterpret_cast<const volatile uint8_t*>(pbStopFlag);   // :79-80
  std::vector<float> oq(4 * (size_t)nC), ot(3 * (size_t)nC), op(3 * (size_t)nP);
  out.cam_q = oq.data(); out.cam_t = ot.data(); out.point = op.data();
  rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
  int rc = rgbl_matcher_acquire(device, &h);
  if (rc == RGBL_OK) {
    rc = rgbl_bundle_adjustment(h, &in, &out);
    rgbl_matcher_release(h);
  }
  if (rc != RGBL_OK) {
    std::cerr << "[BundleAdjustment] " << rgbl_last_error() << std::endl;
    return false;
  }

  // :285-365
  const bool initialisation = nLoopKF == pMap->GetOriginKF()->mnId;
  for (int c = 0; c < nC; ++c) {
    KeyFrameT* pKF = cams[(size_t)c];
    const auto Tcw = pKF->GetPose();
    typedef typename std::decay<decltype(Tcw)>::type SE3T;
    typedef typename std::decay<decltype(Tcw.unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(Tcw.translation())>::type Vec3T;
    const float* cq = oq.data() + 4 * (size_t)c;
    const float* ct = ot.data() + 3 * (size_t)c;
    const SE3T T(QuatT(cq[3], cq[0], cq[1], cq[2]), Vec3T(ct[0], ct[1], ct[2]));
    if (initialisation) pKF->SetPose(T);
    else {
      pKF->mTcwGBA = T;
      pKF->mnBAGlobalForKF = nLoopKF;
    }
  }
  // :368-389
  for (int p = 0; p < nP; ++p) {
    if (!included[(size_t)p]) continue;
    MapPointT* pMP = pts[(size_t)p];
    typedef typename std::decay<decltype(pMP->GetWorldPos())>::type Vec3T;
    const Vec3T X(op[3 * (size_t)p], op[3 * (size_t)p + 1], op[3 * (size_t)p + 2]);
    if (initialisation) {
      pMP->SetWorldPos(X);
      pMP->UpdateNormalAndDepth();
    } else {
      pMP->mPosGBA = X;
      pMP->mnBAGlobalForKF = nLoopKF;
    }
  }
  return true;
}

// :52-57
template <class MapT>
bool GlobalBundleAdjustemnt(MapT* pMap, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0, const bool bRobust = true,
                            int device = 0) {
  const auto vpKFs = pMap->GetAllKeyFrames();
  const auto vpMP = pMap->GetAllMapPoints();
  return BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, device);
}

}  // namespace rgbl_shim
