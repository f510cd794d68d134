// pose_opt_shim_test.cpp — the drop-in rgbl_shim::PoseOptimization (orb_slam3_rgbl_amd/shim/PoseOptimizer.h) on stand-in Frame /
// MapPoint / Sophus types of its own.
//   usage: pose_opt_shim_test <case.bin> <out.bin>
// case.bin (tests/test_pose_opt_shim.py writes it): n, n_levels, then mp_index, world_pos (per feature, zeros without a point),
// xy, octave, uright, q (x y z w), t, K, bf, inv_level_sigma2.
// Variants: host arrays; a resident frame (Frame::mpDeviceFrame) with a DeviceLocalMap in which half of the points are
// registered beforehand; a rig frame and a fisheye camera (refused: -1, pose and flags untouched).  The two device variants must
// leave the same pose, flags and return value; out.bin carries them for the Python side, which holds them to the C ABI's host
// build, the float64 model and the planted pose.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/ORBmatcher.h"
#include "../orb_slam3_rgbl_amd/shim/PoseOptimizer.h"

namespace {

struct V3 {
  float v[3];
  V3() : v{0, 0, 0} {}
  V3(float x, float y, float z) : v{x, y, z} {}
  float operator()(int i) const { return v[i]; }
};
struct Quat {   // Eigen::Quaternionf's constructor order: w, x, y, z
  float c[4];
  Quat() : c{0, 0, 0, 1} {}
  Quat(float w, float x, float y, float z) : c{x, y, z, w} {}
  float x() const { return c[0]; }
  float y() const { return c[1]; }
  float z() const { return c[2]; }
  float w() const { return c[3]; }
};
struct SE3 {
  Quat q; V3 t;
  SE3() {}
  SE3(const Quat& q_, const V3& t_) : q(q_), t(t_) {}
  Quat unit_quaternion() const { return q; }
  V3 translation() const { return t; }
};
struct Camera {
  unsigned type = 0;   // GeometricCamera::CAM_PINHOLE
  unsigned GetType() const { return type; }
};
struct MapPoint {
  static std::mutex mGlobalMutex;
  V3 pos;
  V3 GetWorldPos() { return pos; }
  V3 GetNormal() { return V3(0, 0, 1); }
  float GetMinDistance() { return 1.0f; }
  float GetMaxDistance() { return 100.0f; }
  cv::Mat GetDescriptor() { return cv::Mat::zeros(1, 32, CV_8U); }
};
std::mutex MapPoint::mGlobalMutex;
struct Frame {
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  std::vector<bool> mvbOutlier;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  Camera* mpCamera = nullptr; Camera* mpCamera2 = nullptr;
  const rgbl_device_frame* mpDeviceFrame = nullptr;
  SE3 Tcw;
  SE3 GetPose() { return Tcw; }
  void SetPose(const SE3& T) { Tcw = T; }
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

bool same_pose(const SE3& a, const SE3& b) { return memcmp(a.q.c, b.q.c, 16) == 0 && memcmp(a.t.v, b.t.v, 12) == 0; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int n = 0, n_levels = 0;
  CHECK(rd(f, &n, 1) && rd(f, &n_levels, 1));
  std::vector<int32_t> mp(n), oct(n);
  std::vector<float> pos(3 * (size_t)n), xy(2 * (size_t)n), ur(n), sigma(n_levels);
  float q[4], t[3], K[4], bf;
  CHECK(rd(f, mp.data(), n) && rd(f, pos.data(), 3 * (size_t)n) && rd(f, xy.data(), 2 * (size_t)n) && rd(f, oct.data(), n) && rd(f, ur.data(), n));
  CHECK(rd(f, q, 4) && rd(f, t, 3) && rd(f, K, 4) && rd(f, &bf, 1) && rd(f, sigma.data(), n_levels));
  fclose(f);

  Camera pinhole, fisheye;
  fisheye.type = 1;   // GeometricCamera::CAM_FISHEYE
  std::vector<MapPoint> points(n);
  Frame base;
  base.N = n;
  base.mvpMapPoints.assign(n, nullptr);
  base.mvKeysUn.resize(n);
  for (int i = 0; i < n; ++i) {
    points[i].pos = V3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    if (mp[i] >= 0) base.mvpMapPoints[i] = &points[i];
    base.mvKeysUn[i].pt.x = xy[2 * i]; base.mvKeysUn[i].pt.y = xy[2 * i + 1]; base.mvKeysUn[i].octave = oct[i];
  }
  base.mvuRight = ur; base.mvInvLevelSigma2 = sigma;
  base.mvbOutlier.assign(n, true);   // stale: the call clears the flag of every feature with a map point, and of no other
  base.fx = K[0]; base.fy = K[1]; base.cx = K[2]; base.cy = K[3]; base.mbf = bf;
  base.mpCamera = &pinhole;
  base.Tcw = SE3(Quat(q[3], q[0], q[1], q[2]), V3(t[0], t[1], t[2]));

  // 1. host arrays
  Frame F1 = base;
  const int r1 = rgbl_shim::PoseOptimization(&F1);
  CHECK(r1 > 0);
  for (int i = 0; i < n; ++i)
    if (mp[i] < 0) CHECK(F1.mvbOutlier[i]);   // untouched
  CHECK(!same_pose(F1.Tcw, base.Tcw));

  // 2. resident frame + DeviceLocalMap, half of the points registered beforehand
  {
    rgbl_device_frame* dev = nullptr;
    CHECK(rgbl_device_frame_create(0, n, &dev) == RGBL_OK);
    std::vector<uint8_t> desc(32 * (size_t)n, 0);
    CHECK(rgbl_device_frame_upload(dev, n, desc.data(), xy.data(), oct.data(), ur.data()) == RGBL_OK);
    rgbl_shim::DeviceLocalMap map(0, 64);
    std::vector<MapPoint*> some;
    for (int i = 0; i < n; i += 2)
      if (mp[i] >= 0) some.push_back(&points[i]);
    CHECK(map.Update(some));
    Frame F2 = base;
    F2.mpDeviceFrame = dev;
    F2.mvKeysUn.assign(n, cv::KeyPoint());   // not read: the resident copy is
    const int r2 = rgbl_shim::PoseOptimization(&F2, &map);
    CHECK(r2 == r1 && same_pose(F2.Tcw, F1.Tcw) && F2.mvbOutlier == F1.mvbOutlier);
    CHECK(map.size() > some.size());          // the other half was uploaded on the spot
    rgbl_device_frame_destroy(dev);
  }

  // 3. fewer than 3 correspondences: 0, the pose stays, the flags of the features with a point are cleared
  {
    Frame F3 = base;
    int kept = 0;
    for (int i = 0; i < n; ++i)
      if (F3.mvpMapPoints[i] && ++kept > 2) F3.mvpMapPoints[i] = nullptr;
    CHECK(rgbl_shim::PoseOptimization(&F3) == 0 && same_pose(F3.Tcw, base.Tcw));
    for (int i = 0; i < n; ++i) CHECK(F3.mvbOutlier[i] == (F3.mvpMapPoints[i] == nullptr));
  }

  // 4. refused: a rig frame, a camera that is not a Pinhole
  {
    Frame F4 = base;
    F4.mpCamera2 = &pinhole;
    CHECK(rgbl_shim::PoseOptimization(&F4) == -1 && same_pose(F4.Tcw, base.Tcw) && F4.mvbOutlier == base.mvbOutlier);
    Frame F5 = base;
    F5.mpCamera = &fisheye;
    CHECK(rgbl_shim::PoseOptimization(&F5) == -1 && same_pose(F5.Tcw, base.Tcw) && F5.mvbOutlier == base.mvbOutlier);
  }

  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  fwrite(&r1, sizeof(int), 1, o);
  fwrite(F1.Tcw.q.c, sizeof(float), 4, o);
  fwrite(F1.Tcw.t.v, sizeof(float), 3, o);
  std::vector<uint8_t> flags(n);
  for (int i = 0; i < n; ++i) flags[i] = F1.mvbOutlier[i] ? 1 : 0;
  fwrite(flags.data(), 1, n, o);
  fclose(o);
  rgbl_matcher_pool_clear();
  printf("POSE_OPT_SHIM_OK %d inliers of %d features\n", r1, n);
  return 0;
}
