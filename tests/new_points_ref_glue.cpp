// new_points_ref_glue.cpp — the reference's own LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:388-712),
// GeometricTools::Triangulate (src/GeometricTools.cc:47-66), KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772),
// Pinhole::unprojectEig and Pinhole::project (src/CameraModels/Pinhole.cpp:61-64, 30-33), UNMODIFIED: tests/new_points_golden.py
// cuts the five definitions out of the reference's sources by signature into new_points_ref_bodies.inc in the build directory
// (never committed) and compiles this file against the stand-in types of new_points_ref_types.h with -O2 -ffp-contract=off.
// Its SearchForTriangulation is the reference's own ORBmatcher.cc through oracle/_ref/libref_orbmatcher.so.  TEST INFRASTRUCTURE.
#include <dlfcn.h>
#include <string.h>

#include "new_points_ref_types.h"

namespace ORB_SLAM3 {
#include "new_points_ref_bodies.inc"
}  // namespace ORB_SLAM3

namespace {
struct KfArrays {   // oracle/ref_matcher_glue.cpp
  int n;
  const uint8_t* desc;
  const float* kp_xy;
  const int* kp_octave;
  const float* kp_angle;
  const float* uright;
  const uint8_t* has_mp;
  int nnodes;
  const int *node_id, *node_off, *node_feat;
};
struct KfIn {
  KfArrays a;
  const float* depth;
  const float* xy_raw;
  float q[4], t[3];
  float median_depth;
};
typedef int (*search_fn)(const KfArrays*, const KfArrays*, const float*, const float*, const float*, int, const float*, const float*,
                         const float*, const float*, int, int, int, int*, float*, float*, float*);
search_fn g_search = nullptr;
struct Flat { const KfIn* in; std::vector<uint8_t> has_mp; };
std::vector<Flat> g_flat;   // [0] the current key frame, [1 + i] neighbour i
const float* g_K = nullptr;

Sophus::SE3<float> pose_of(const float q[4], const float t[3]) {
  return Sophus::SE3<float>(Sophus::SE3Core<float>(Eigen::Quaternionf(q[3], q[0], q[1], q[2]), Eigen::Vector3f(t[0], t[1], t[2])));
}
void fill(ORB_SLAM3::KeyFrame& kf, const KfIn& in, ORB_SLAM3::Pinhole* cam, ORB_SLAM3::MapPoint* some, const float* K, float mb, float mbf,
          const float* sf, const float* s2, int n_levels, float scale_factor) {
  const int n = in.a.n;
  kf.N = n;
  kf.mpCamera = cam;
  kf.fx = K[0]; kf.fy = K[1]; kf.cx = K[2]; kf.cy = K[3];
  kf.invfx = 1.0f / kf.fx; kf.invfy = 1.0f / kf.fy;   // Frame.cc
  kf.mb = mb; kf.mbf = mbf; kf.mfScaleFactor = scale_factor; kf.median_depth = in.median_depth;
  kf.mvKeysUn.resize(n); kf.mvKeys.resize(n); kf.mvpMapPoints.resize(n);
  kf.mvuRight.assign(in.a.uright, in.a.uright + n);
  kf.mvDepth.assign(in.depth, in.depth + n);
  for (int i = 0; i < n; ++i) {
    kf.mvKeysUn[i].pt = cv::Point2f(in.a.kp_xy[2 * i], in.a.kp_xy[2 * i + 1]);
    kf.mvKeysUn[i].octave = in.a.kp_octave[i];
    kf.mvKeysUn[i].angle = in.a.kp_angle[i];
    kf.mvKeys[i] = kf.mvKeysUn[i];
    kf.mvKeys[i].pt = cv::Point2f(in.xy_raw[2 * i], in.xy_raw[2 * i + 1]);
    kf.mvpMapPoints[i] = in.a.has_mp[i] ? some : nullptr;
  }
  kf.mvScaleFactors.assign(sf, sf + n_levels);
  kf.mvLevelSigma2.assign(s2, s2 + n_levels);
  kf.mTcw = pose_of(in.q, in.t);            // KeyFrame::SetPose (KeyFrame.cc:107-120)
  kf.mTwc = Sophus::SE3<float>(kf.mTcw.inverse());
  kf.mRwc = kf.mTwc.rotationMatrix();
}
}  // namespace

int ORB_SLAM3::ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t> >& vMatchedPairs,
                                                  const bool bOnlyStereo, const bool bCoarse) {
  Flat &f1 = g_flat[0], &f2 = g_flat[1 + pKF2->index];
  for (int i = 0; i < pKF1->N; ++i) f1.has_mp[i] = pKF1->mvpMapPoints[i] ? 1 : 0;   // the map points as they are NOW
  for (int i = 0; i < pKF2->N; ++i) f2.has_mp[i] = pKF2->mvpMapPoints[i] ? 1 : 0;
  KfArrays a1 = f1.in->a, a2 = f2.in->a;
  a1.has_mp = f1.has_mp.data(); a2.has_mp = f2.has_mp.data();
  std::vector<int> m12((size_t)pKF1->N + 1, -1);
  float R12[9], t12[3], ep[2];
  const int nm = g_search(&a1, &a2, g_K, pKF2->mvScaleFactors.data(), pKF2->mvLevelSigma2.data(), (int)pKF2->mvScaleFactors.size(), f1.in->q,
                          f1.in->t, f2.in->q, f2.in->t, bOnlyStereo, bCoarse, 0, m12.data(), R12, t12, ep);
  vMatchedPairs.clear();
  for (int i = 0; i < pKF1->N; ++i)
    if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
  return nm;
}

#pragma GCC visibility push(default)   // the rest is hidden: the matcher library defines an ORB_SLAM3::ORBmatcher of its own
extern "C" {

int ref_np_open_matcher(const char* path) {
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return -1;
  g_search = (search_fn)dlsym(h, "ref_search_triangulation");
  return g_search ? 0 : -2;
}

// what the stand-in Sophus arithmetic makes of a pose: matrix3x4() of Tcw and the camera centre; and of a pair: R12, t12 and the
// epipole as ORBmatcher.cc:914-931 computes them
void ref_np_pose(const float q[4], const float t[3], float Tcw[12], float Ow[3]) {
  const Sophus::SE3<float> T = pose_of(q, t);
  memcpy(Tcw, T.matrix3x4().m, sizeof(float) * 12);
  const Sophus::SE3<float> Twc(T.inverse());
  for (int i = 0; i < 3; ++i) Ow[i] = Twc.translation()(i);
}
void ref_np_pair(const float q1[4], const float t1[3], const float q2[4], const float t2[3], const float K[4], float R12[9], float t12[3], float ep[2]) {
  const Sophus::SE3<float> T1 = pose_of(q1, t1), T2 = pose_of(q2, t2);
  const Sophus::SE3Core<float> T12 = T1 * T2.inverse();
  const Eigen::Matrix3f R = T12.rotationMatrix();
  memcpy(R12, R.m, sizeof(float) * 9);
  for (int i = 0; i < 3; ++i) t12[i] = T12.translation()(i);
  const Eigen::Vector3f C2 = T2 * Sophus::SE3<float>(T1.inverse()).translation();
  ep[0] = K[0] * C2[0] / C2[2] + K[2];
  ep[1] = K[1] * C2[1] / C2[2] + K[3];
}

// LocalMapping::CreateNewMapPoints on stand-in objects.  out_idx: (neighbour, idx1, idx2) and out_x3D: the world position of
// every MapPoint of mlpRecentAddedMapPoints, in list order.  Returns how many there are (at most cap are written).
int ref_create_new_map_points(const KfIn* kf1, int nn, const KfIn* kf2, const float K[4], float mb, float mbf, const float* sf,
                              const float* s2, int n_levels, float scale_factor, int monocular, int inertial, int far_points,
                              float th_far_points, int cap, int32_t* out_idx, float* out_x3D) {
  using namespace ORB_SLAM3;
  if (!g_search) return -1;
  Pinhole cam;
  cam.mvParameters.assign(K, K + 4);
  MapPoint some(Eigen::Vector3f(), nullptr, nullptr);
  KeyFrame cur;
  std::vector<KeyFrame> neigh((size_t)nn);
  g_flat.clear();
  g_flat.push_back(Flat{kf1, std::vector<uint8_t>((size_t)kf1->a.n + 1)});
  g_K = K;
  fill(cur, *kf1, &cam, &some, K, mb, mbf, sf, s2, n_levels, scale_factor);
  for (int i = 0; i < nn; ++i) {
    fill(neigh[i], kf2[i], &cam, &some, K, mb, mbf, sf, s2, n_levels, scale_factor);
    neigh[i].index = i;
    cur.neighbours.push_back(&neigh[i]);
    g_flat.push_back(Flat{kf2 + i, std::vector<uint8_t>((size_t)kf2[i].a.n + 1)});
  }
  Tracking tracker;
  Atlas atlas;
  LocalMapping lm;
  lm.mbMonocular = monocular != 0; lm.mbInertial = inertial != 0; lm.mbFarPoints = far_points != 0; lm.mThFarPoints = th_far_points;
  lm.mpCurrentKeyFrame = &cur; lm.mpTracker = &tracker; lm.mpAtlas = &atlas;
  lm.CreateNewMapPoints();
  int k = 0;
  for (MapPoint* p : lm.mlpRecentAddedMapPoints) {
    if (k < cap) {
      out_idx[3 * k] = p->mObs[1].first->index; out_idx[3 * k + 1] = p->mObs[0].second; out_idx[3 * k + 2] = p->mObs[1].second;
      for (int c = 0; c < 3; ++c) out_x3D[3 * k + c] = p->mWorldPos(c);
    }
    ++k;
    delete p;
  }
  return k;
}

}  // extern "C"
#pragma GCC visibility pop
