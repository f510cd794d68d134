// LocalBundleAdjuster.h — drop-in for void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap,
// int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges) (include/Optimizer.h, src/Optimizer.cc:1116-1498) on the
// device: the graph walk (:1118-1186) and the edge loop (:1282-1403) on the host as the reference runs them, ONE
// rgbl_local_bundle_adjustment call for :1188-1411, then :1413-1497 in the reference's order.  INTEGRATION.md shows the line of
// LocalMapping.cc that changes.
//
// Reads of a key frame mnId, mnBALocalForKF, mnBAFixedForKF (written as the reference writes them), isBad(), GetMap(),
// GetVectorCovisibleKeyFrames(), GetMapPointMatches(), GetPose(), mvKeysUn, mvuRight, mvInvLevelSigma2, mpCamera, mpCamera2,
// fx, fy, cx, cy, mbf; of a map point mnBALocalForKF, isBad(), GetMap(), GetObservations(), GetWorldPos(); of the map
// GetInitKFid(), IsInertial(), mMutexMapUpdate.  Writes, when the call ran: EraseMapPointMatch / EraseObservation for the
// erase list (monocular edges first, then stereo: the order of :1417-1460) under the map's mutex, SetPose of every local key
// frame, SetWorldPos of every local point and pMap->IncreaseChangeIndex().  The per-point UpdateNormalAndDepth (:1494) runs on
// the host, or, with a DeviceLocalMap, as ONE Refresh(moved, true, false) on the device.  num_MPs is not written (the
// reference does not write it either); msOptKFs / msFixedKFs (debug sets) are not kept.
//
// The edge order is the reference's: point-major in lLocalMapPoints order, within a point in the order of its observations map
// (std::map<KeyFrame*, ...>: by pointer).  A monocular edge reads K from mpCamera->getParameter(0 .. 3), a stereo edge from
// fx, fy, cx, cy and mbf (:1323, :1352-1356).
//
// Returns true when the reference's work was done here (also at its two early returns).  false, with NOTHING written beyond the
// marks of the walk: a key frame with a second camera (the rig edge :1366-1400), a camera that is not a Pinhole, a key frame
// whose monocular and stereo intrinsics differ, a limit of the C ABI exceeded, or a failed call (message on stderr) - the
// caller then runs Optimizer::LocalBundleAdjustment.
#pragma once
#include <string.h>

#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace rgbl_shim {

struct NoLocalMap {};   // the host runs UpdateNormalAndDepth per point

template <class KeyFrameT, class MapT, class LocalMapT = NoLocalMap>
bool LocalBundleAdjustment(KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges,
                           LocalMapT* pLocalMap = nullptr, int device = 0) {
  typedef typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type>::type MapPointT;
  (void)num_MPs;
  // :1118-1132
  std::list<KeyFrameT*> lLocalKeyFrames;
  lLocalKeyFrames.push_back(pKF);
  pKF->mnBALocalForKF = pKF->mnId;
  auto* pCurrentMap = pKF->GetMap();
  const std::vector<KeyFrameT*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  for (KeyFrameT* pKFi : vNeighKFs) {
    pKFi->mnBALocalForKF = pKF->mnId;
    if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
  }
  // :1134-1160
  num_fixedKF = 0;
  std::list<MapPointT*> lLocalMapPoints;
  for (KeyFrameT* pKFi : lLocalKeyFrames) {
    if (pKFi->mnId == pMap->GetInitKFid()) num_fixedKF = 1;
    const std::vector<MapPointT*> vpMPs = pKFi->GetMapPointMatches();
    for (MapPointT* pMP : vpMPs)
      if (pMP && !pMP->isBad() && pMP->GetMap() == pCurrentMap && pMP->mnBALocalForKF != pKF->mnId) {
        lLocalMapPoints.push_back(pMP);
        pMP->mnBALocalForKF = pKF->mnId;
      }
  }
  // :1162-1186
  std::list<KeyFrameT*> lFixedCameras;
  for (MapPointT* pMP : lLocalMapPoints) {
    const auto observations = pMP->GetObservations();
    for (const auto& ob : observations) {
      KeyFrameT* pKFi = ob.first;
      if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
        pKFi->mnBAFixedForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
      }
    }
  }
  num_fixedKF = (int)lFixedCameras.size() + num_fixedKF;
  if (num_fixedKF == 0) return true;   // :1182-1186

  // the vertices (:1213-1243): free cameras in list order, then the fixed ones
  std::vector<KeyFrameT*> cams(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
  const int n_free = (int)cams.size();
  cams.insert(cams.end(), lFixedCameras.begin(), lFixedCameras.end());
  const int nC = (int)cams.size();
  std::map<KeyFrameT*, int> index;
  std::vector<uint8_t> free_is_fixed((size_t)n_free, 0);
  std::vector<float> q(4 * (size_t)nC), t(3 * (size_t)nC), K(4 * (size_t)nC), bf((size_t)nC);
  for (int c = 0; c < nC; ++c) {
    KeyFrameT* k = cams[(size_t)c];
    index[k] = c;
    if (k->mpCamera2) { std::cerr << "[LocalBundleAdjustment] two-camera key frames are not covered by the device path" << std::endl; return false; }
    if (k->mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) { std::cerr << "[LocalBundleAdjustment] only Pinhole cameras are covered by the device path" << std::endl; return false; }
    const float Kc[4] = {k->fx, k->fy, k->cx, k->cy};
    for (int i = 0; i < 4; ++i) {
      if (k->mpCamera->getParameter(i) != Kc[i]) { std::cerr << "[LocalBundleAdjustment] a key frame's camera and its fx, fy, cx, cy differ" << std::endl; return false; }
      K[4 * (size_t)c + i] = Kc[i];
    }
    bf[(size_t)c] = k->mbf;
    const auto Tcw = k->GetPose();
    const auto uq = Tcw.unit_quaternion();
    const auto tr = Tcw.translation();
    q[4 * (size_t)c] = uq.x(); q[4 * (size_t)c + 1] = uq.y(); q[4 * (size_t)c + 2] = uq.z(); q[4 * (size_t)c + 3] = uq.w();
    for (int i = 0; i < 3; ++i) t[3 * (size_t)c + i] = tr(i);
    if (c < n_free) free_is_fixed[(size_t)c] = k->mnId == pMap->GetInitKFid() ? 1 : 0;   // :1220
  }
  num_OptKF = n_free;   // :1227

  // the points and the edges (:1282-1403)
  std::vector<MapPointT*> pts(lLocalMapPoints.begin(), lLocalMapPoints.end());
  const int nP = (int)pts.size();
  std::vector<float> pos(3 * (size_t)nP), obs, info;
  std::vector<int32_t> edge_point, edge_cam;
  std::vector<KeyFrameT*> edge_kf;
  for (int p = 0; p < nP; ++p) {
    const auto X = pts[(size_t)p]->GetWorldPos();
    for (int i = 0; i < 3; ++i) pos[3 * (size_t)p + i] = X(i);
    const auto observations = pts[(size_t)p]->GetObservations();
    for (const auto& ob : observations) {
      KeyFrameT* pKFi = ob.first;
      if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;
      const int leftIndex = std::get<0>(ob.second);
      if (leftIndex == -1) continue;
      const float ur = pKFi->mvuRight[(size_t)leftIndex];
      if (!(ur < 0) && !(ur >= 0)) continue;   // :1305 / :1332: neither branch takes a NaN
      const auto it = index.find(pKFi);
      if (it == index.end()) { std::cerr << "[LocalBundleAdjustment] an observation in a key frame without a vertex" << std::endl; return false; }
      const auto& kpUn = pKFi->mvKeysUn[(size_t)leftIndex];
      edge_point.push_back(p); edge_cam.push_back(it->second); edge_kf.push_back(pKFi);
      obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(ur < 0 ? -1.0f : ur);
      info.push_back(pKFi->mvInvLevelSigma2[(size_t)kpUn.octave]);
    }
  }
  const int nE = (int)edge_point.size();
  num_edges = nE;   // :1404

  rgbl_lba_input in;
  rgbl_lba_output out;
  memset(&in, 0, sizeof(in));
  memset(&out, 0, sizeof(out));
  in.n_free = n_free; in.n_fixed = nC - n_free; in.free_is_fixed = free_is_fixed.data();
  in.cam_q = q.data(); in.cam_t = t.data(); in.cam_K = K.data(); in.cam_bf = bf.data();
  in.n_points = nP; in.world_pos = pos.data();
  in.n_edges = nE; in.edge_point = edge_point.data(); in.edge_cam = edge_cam.data(); in.edge_obs = obs.data(); in.edge_inv_sigma2 = info.data();
  in.max_iterations = 10;                                        // :1411
  in.user_lambda_init = pMap->IsInertial() ? 100.0 : 0.0;        // :1197-1198
  static_assert(sizeof(bool) == 1, "pbStopFlag is read as one byte");
  in.stop_byte = reinterpret_cast<const volatile uint8_t*>(pbStopFlag);   // :1203-1204, :1406-1408
  std::vector<float> oq(4 * (size_t)n_free), ot(3 * (size_t)n_free), op(3 * (size_t)nP);
  std::vector<uint8_t> flags((size_t)nE, 0);
  out.cam_q = oq.data(); out.cam_t = ot.data(); out.point = op.data(); out.flags = flags.data();
  rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's
  int rc = rgbl_matcher_acquire(device, &h);
  if (rc == RGBL_OK) {
    rc = rgbl_local_bundle_adjustment(h, &in, &out);
    rgbl_matcher_release(h);
  }
  if (rc != RGBL_OK) {
    std::cerr << "[LocalBundleAdjustment] " << rgbl_last_error() << std::endl;
    return false;
  }
  if (!out.diag.ran) return true;   // :1406-1408

  // :1413-1460: monocular edges first, then stereo
  std::vector<std::pair<KeyFrameT*, MapPointT*>> vToErase;
  for (int stereo = 0; stereo < 2; ++stereo)
    for (int k = 0; k < nE; ++k) {
      if ((obs[3 * (size_t)k + 2] < 0 ? 0 : 1) != stereo) continue;
      MapPointT* pMP = pts[(size_t)edge_point[(size_t)k]];
      if (pMP->isBad()) continue;
      if (flags[(size_t)k] & 1) vToErase.push_back(std::make_pair(edge_kf[(size_t)k], pMP));
    }
  std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // :1464
  for (auto& e : vToErase) {
    e.first->EraseMapPointMatch(e.second);
    e.second->EraseObservation(e.first);
  }
  // :1479-1486
  for (int c = 0; c < n_free; ++c) {
    const auto Tcw = cams[(size_t)c]->GetPose();
    typedef typename std::decay<decltype(Tcw)>::type SE3T;
    typedef typename std::decay<decltype(Tcw.unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(Tcw.translation())>::type Vec3T;
    const float* cq = oq.data() + 4 * (size_t)c;
    const float* ct = ot.data() + 3 * (size_t)c;
    cams[(size_t)c]->SetPose(SE3T(QuatT(cq[3], cq[0], cq[1], cq[2]), Vec3T(ct[0], ct[1], ct[2])));
  }
  // :1489-1495
  for (int p = 0; p < nP; ++p) {
    typedef typename std::decay<decltype(pts[(size_t)p]->GetWorldPos())>::type Vec3T;
    pts[(size_t)p]->SetWorldPos(Vec3T(op[3 * (size_t)p], op[3 * (size_t)p + 1], op[3 * (size_t)p + 2]));
    if constexpr (std::is_same<LocalMapT, NoLocalMap>::value) pts[(size_t)p]->UpdateNormalAndDepth();
  }
  if constexpr (!std::is_same<LocalMapT, NoLocalMap>::value) {
    if (!pLocalMap || !pLocalMap->Refresh(pts, true, false))
      for (MapPointT* pMP : pts) pMP->UpdateNormalAndDepth();
  }
  pMap->IncreaseChangeIndex();   // :1497
  return true;
}

}  // namespace rgbl_shim
