// PoseOptimizer.h — drop-in for int Optimizer::PoseOptimization(Frame* pFrame) (include/Optimizer.h, src/Optimizer.cc:814-1114) on
// the device: one rgbl_pose_optimization call.  INTEGRATION.md shows the lines of Tracking.cc that change.
//
// Reads pFrame->mvpMapPoints, mvKeysUn, mvuRight, mvInvLevelSigma2, fx, fy, cx, cy, mbf and GetPose(); writes mvbOutlier (where
// there is a map point) and SetPose(), and returns the reference's value.  The frame's resident copy (Frame::mpDeviceFrame,
// LocalMap.h) is used when it is there, and with a DeviceLocalMap the positions come from the map points' slots - a point
// without one is uploaded on the spot - so the matches never leave the card between the search and the pose.
//
// Single-camera pinhole frames only: a rig frame (mpCamera2 != nullptr, Optimizer.cc:930-991) or a camera that is not a Pinhole
// (GeometricCamera::CAM_PINHOLE) is refused with a message, returns -1 and leaves the frame untouched.
#pragma once
#include <iostream>
#include <mutex>
#include <type_traits>
#include <vector>

#include "LocalMap.h"

namespace rgbl_shim {

template <class FrameT>
int PoseOptimization(FrameT* pFrame, DeviceLocalMap* pMap = nullptr, int device = 0) {
  typedef typename std::remove_pointer<typename std::decay<decltype(pFrame->mvpMapPoints[0])>::type>::type MapPointT;
  if (pFrame->mpCamera2) {
    std::cerr << "[PoseOptimization] fisheye stereo rigs (mpCamera2) are not covered by the device path" << std::endl;
    return -1;
  }
  if (pFrame->mpCamera->GetType() != 0u /* GeometricCamera::CAM_PINHOLE */) {
    std::cerr << "[PoseOptimization] only Pinhole cameras are covered by the device path" << std::endl;
    return -1;
  }
  const int N = pFrame->N;
  std::vector<int32_t> mp((size_t)N, -1), slot, oct;
  std::vector<float> pos, xy;
  std::vector<MapPointT*> vpMPs, vpNew;
  std::vector<int> vnNew;
  struct SearchBracket {   // as ORBmatcher::SearchLocalPoints: slots erased meanwhile are not handed to other points
    DeviceLocalMap* p;
    explicit SearchBracket(DeviceLocalMap* q) : p(q) { if (p) p->BeginSearch(); }
    ~SearchBracket() { if (p) p->EndSearch(); }
  } bracket(pMap);
  {
    std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);   // Optimizer.cc:856
    for (int i = 0; i < N; ++i) {
      MapPointT* pMP = pFrame->mvpMapPoints[i];
      if (!pMP) continue;
      mp[i] = (int32_t)vpMPs.size();
      vpMPs.push_back(pMP);
      if (pMap) {
        slot.push_back(pMap->SlotOf(pMP));
        if (slot.back() < 0) { vpNew.push_back(pMP); vnNew.push_back((int)slot.size() - 1); }
      } else {
        const auto P = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) pos.push_back(P(k));
      }
    }
  }
  if (!vpNew.empty()) {
    std::vector<int32_t> vnSlots;
    if (!pMap->Update(vpNew, &vnSlots)) return -1;
    for (size_t k = 0; k < vnNew.size(); ++k) slot[vnNew[k]] = vnSlots[k];
  }
  rgbl_pose_opt_input in{};
  in.n = N; in.mp_index = mp.data(); in.n_points = (int)vpMPs.size();
  if (pMap) { in.pool = pMap->handle(); in.slot = slot.data(); }
  else in.world_pos = pos.data();
  in.device = device_frame_of(*pFrame, 0);
  if (!in.device) {
    xy.resize(2 * (size_t)N); oct.resize((size_t)N);
    for (int i = 0; i < N; ++i) {
      xy[2 * (size_t)i] = pFrame->mvKeysUn[i].pt.x;
      xy[2 * (size_t)i + 1] = pFrame->mvKeysUn[i].pt.y;
      oct[i] = pFrame->mvKeysUn[i].octave;
    }
    in.kp_xy = xy.data(); in.kp_octave = oct.data(); in.uright = pFrame->mvuRight.data();
  }
  const auto Tcw = pFrame->GetPose();
  const auto q = Tcw.unit_quaternion();
  const auto t = Tcw.translation();
  in.Tcw_q[0] = q.x(); in.Tcw_q[1] = q.y(); in.Tcw_q[2] = q.z(); in.Tcw_q[3] = q.w();
  for (int k = 0; k < 3; ++k) in.Tcw_t[k] = t(k);
  in.K[0] = pFrame->fx; in.K[1] = pFrame->fy; in.K[2] = pFrame->cx; in.K[3] = pFrame->cy;
  in.bf = pFrame->mbf;
  in.inv_level_sigma2 = pFrame->mvInvLevelSigma2.data();
  in.n_levels = (int)pFrame->mvInvLevelSigma2.size();
  std::vector<uint8_t> outlier((size_t)(N > 0 ? N : 1), 0);
  rgbl_pose_opt_output out{};
  out.outlier = outlier.data();
  rgbl_matcher* h = nullptr;   // from the library's pool, as the drop-in ORBmatcher's: no stream or arena is created per call
  if (rgbl_matcher_acquire(device, &h) != RGBL_OK) {
    std::cerr << "[PoseOptimization] " << rgbl_last_error() << std::endl;
    return -1;
  }
  const int rc = rgbl_pose_optimization(h, &in, &out);
  rgbl_matcher_release(h);
  if (rc != RGBL_OK) {
    std::cerr << "[PoseOptimization] " << rgbl_last_error() << std::endl;
    return -1;
  }
  for (int i = 0; i < N; ++i)
    if (mp[i] >= 0) pFrame->mvbOutlier[i] = outlier[i] != 0;   // :869 / :897 and :1030-1095
  if (out.diag.rounds > 0) {                                   // :996-997 return before SetPose
    typedef typename std::decay<decltype(Tcw)>::type SE3T;
    typedef typename std::decay<decltype(q)>::type QuatT;
    typedef typename std::decay<decltype(t)>::type Vec3T;
    pFrame->SetPose(SE3T(QuatT(out.Tcw_q[3], out.Tcw_q[0], out.Tcw_q[1], out.Tcw_q[2]), Vec3T(out.Tcw_t[0], out.Tcw_t[1], out.Tcw_t[2])));
  }
  return out.result;
}

}  // namespace rgbl_shim
