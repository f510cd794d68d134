// gba_shim_test.cpp — the drop-ins rgbl_shim::BundleAdjustment / GlobalBundleAdjustemnt
// (orb_slam3_rgbl_amd/shim/GlobalBundleAdjuster.h) on stand-in KeyFrame / MapPoint / Map types of its own.
//   usage: gba_shim_test <scene.bin> <out.bin>
// scene.bin (tests/test_gba_shim.py writes it): n_kf, n_mp, init_id, origin (index of the origin key frame), stop, nLoopKF,
// robust, iterations, through_map; per key frame id, bad, second_camera, q (x y z w), t, K, bf, n_features and per feature x, y,
// octave, uright, map point (-1: none); per map point id, bad, pos; n_extra and that many (key frame, map point) observations
// whose left index is -1; the key frames of vpKFs (count, then indices) and the points of vpMP likewise; the 8 entries of
// mvInvLevelSigma2.  All key frames live in ONE array, so the pointer-ordered observations maps are ordered by index.
// out.bin: the drop-in's return value; per key frame its pose, SetPose count, mTcwGBA, mnBAGlobalForKF; per map point its
// position, SetWorldPos and UpdateNormalAndDepth counts, mPosGBA, mnBAGlobalForKF.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/GlobalBundleAdjuster.h"

namespace {
struct V3 {
  float v[3] = {0, 0, 0};
  V3() {}
  V3(float a, float b, float c) { v[0] = a; v[1] = b; v[2] = c; }
  float operator()(int i) const { return v[i]; }
};
struct Quat {
  float c[4] = {0, 0, 0, 1};   // x y z w
  Quat() {}
  Quat(float w, float x, float y, float z) { c[0] = x; c[1] = y; c[2] = z; c[3] = w; }
  float x() const { return c[0]; } float y() const { return c[1]; } float z() const { return c[2]; } float w() const { return c[3]; }
};
struct SE3 {
  Quat q; V3 t;
  SE3() {}
  SE3(const Quat& qq, const V3& tt) : q(qq), t(tt) {}
  Quat unit_quaternion() const { return q; }
  V3 translation() const { return t; }
};
struct Camera {
  float K[4];
  unsigned GetType() const { return 0u; }
  float getParameter(int i) const { return K[i]; }
};
struct Pt { float x, y; };
struct KeyPoint { Pt pt; int octave; };
struct KeyFrame;
struct MapPoint;
struct Map {
  long unsigned init_id = 0;
  KeyFrame* origin = nullptr;
  std::vector<KeyFrame*> all_kfs;
  std::vector<MapPoint*> all_mps;
  long unsigned GetInitKFid() { return init_id; }
  KeyFrame* GetOriginKF() { return origin; }
  std::vector<KeyFrame*> GetAllKeyFrames() { return all_kfs; }
  std::vector<MapPoint*> GetAllMapPoints() { return all_mps; }
};
struct MapPoint {
  long unsigned mnId = 0, mnBAGlobalForKF = 0;
  V3 pos, mPosGBA;
  bool bad = false;
  std::map<KeyFrame*, std::tuple<int, int>> obs;
  int set_pos = 0, updated = 0;
  bool isBad() { return bad; }
  V3 GetWorldPos() { return pos; }
  void SetWorldPos(const V3& p) { pos = p; ++set_pos; }
  void UpdateNormalAndDepth() { ++updated; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return obs; }
};
struct KeyFrame {
  long unsigned mnId = 0, mnBAGlobalForKF = 0;
  bool bad = false;
  Map* map = nullptr;
  SE3 pose, mTcwGBA;
  int set_pose = 0;
  Camera cam;
  Camera* mpCamera = &cam;
  Camera* mpCamera2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  SE3 GetPose() { return pose; }
  void SetPose(const SE3& T) { pose = T; ++set_pose; }
};

template <class T> T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short scene file\n"); exit(2); } return v; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int n_kf = rd<int>(f), n_mp = rd<int>(f), init_id = rd<int>(f), origin = rd<int>(f), stop = rd<int>(f), loop_kf = rd<int>(f),
            robust = rd<int>(f), iterations = rd<int>(f), through_map = rd<int>(f);
  Map map;
  map.init_id = (long unsigned)init_id;
  std::vector<KeyFrame> kfs((size_t)n_kf);   // ONE array: pointer order is index order
  std::vector<MapPoint> mps((size_t)n_mp);
  std::vector<std::vector<int>> feat_mp((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[(size_t)k];
    K.map = &map;
    K.mpCamera = &K.cam;
    K.mnId = (long unsigned)rd<int>(f); K.bad = rd<int>(f) != 0;
    if (rd<int>(f)) K.mpCamera2 = &K.cam;
    float q[4], t[3];
    for (float& v : q) v = rd<float>(f);
    for (float& v : t) v = rd<float>(f);
    K.pose = SE3(Quat(q[3], q[0], q[1], q[2]), V3(t[0], t[1], t[2]));
    for (int i = 0; i < 4; ++i) K.cam.K[i] = rd<float>(f);
    K.fx = K.cam.K[0]; K.fy = K.cam.K[1]; K.cx = K.cam.K[2]; K.cy = K.cam.K[3];
    K.mbf = rd<float>(f);
    const int nf = rd<int>(f);
    for (int i = 0; i < nf; ++i) {
      KeyPoint kp; kp.pt.x = rd<float>(f); kp.pt.y = rd<float>(f); kp.octave = rd<int>(f);
      K.mvKeysUn.push_back(kp); K.mvuRight.push_back(rd<float>(f));
      feat_mp[(size_t)k].push_back(rd<int>(f));
    }
  }
  map.origin = &kfs[(size_t)origin];
  for (int p = 0; p < n_mp; ++p) {
    MapPoint& M = mps[(size_t)p];
    M.mnId = (long unsigned)rd<int>(f); M.bad = rd<int>(f) != 0;
    const float x = rd<float>(f), y = rd<float>(f), z = rd<float>(f);
    M.pos = V3(x, y, z);
  }
  const int n_extra = rd<int>(f);
  std::vector<std::pair<int, int>> extra;
  for (int i = 0; i < n_extra; ++i) { const int k = rd<int>(f), p = rd<int>(f); extra.push_back(std::make_pair(k, p)); }
  std::vector<KeyFrame*> vpKFs;
  std::vector<MapPoint*> vpMP;
  const int n_list_kf = rd<int>(f);
  for (int i = 0; i < n_list_kf; ++i) vpKFs.push_back(&kfs[(size_t)rd<int>(f)]);
  const int n_list_mp = rd<int>(f);
  for (int i = 0; i < n_list_mp; ++i) vpMP.push_back(&mps[(size_t)rd<int>(f)]);
  std::vector<float> sigma;
  for (int i = 0; i < 8; ++i) sigma.push_back(rd<float>(f));
  fclose(f);
  for (int k = 0; k < n_kf; ++k) {
    kfs[(size_t)k].mvInvLevelSigma2 = sigma;
    for (size_t i = 0; i < feat_mp[(size_t)k].size(); ++i) {
      const int p = feat_mp[(size_t)k][i];
      if (p >= 0) mps[(size_t)p].obs[&kfs[(size_t)k]] = std::make_tuple((int)i, -1);
    }
  }
  for (auto& e : extra) mps[(size_t)e.second].obs[&kfs[(size_t)e.first]] = std::make_tuple(-1, 0);
  map.all_kfs = vpKFs; map.all_mps = vpMP;
  bool flag = stop != 0;
  const bool done = through_map ? rgbl_shim::GlobalBundleAdjustemnt(&map, iterations, &flag, (unsigned long)loop_kf, robust != 0)
                                : rgbl_shim::BundleAdjustment(vpKFs, vpMP, iterations, &flag, (unsigned long)loop_kf, robust != 0);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int head = done ? 1 : 0;
  fwrite(&head, sizeof(int), 1, o);
  for (KeyFrame& K : kfs) {
    const float v[16] = {K.pose.q.c[0], K.pose.q.c[1], K.pose.q.c[2], K.pose.q.c[3], K.pose.t.v[0], K.pose.t.v[1], K.pose.t.v[2], (float)K.set_pose,
                         K.mTcwGBA.q.c[0], K.mTcwGBA.q.c[1], K.mTcwGBA.q.c[2], K.mTcwGBA.q.c[3], K.mTcwGBA.t.v[0], K.mTcwGBA.t.v[1], K.mTcwGBA.t.v[2],
                         (float)K.mnBAGlobalForKF};
    fwrite(v, sizeof(float), 16, o);
  }
  for (MapPoint& M : mps) {
    const float v[9] = {M.pos.v[0], M.pos.v[1], M.pos.v[2], (float)M.set_pos, (float)M.updated, M.mPosGBA.v[0], M.mPosGBA.v[1], M.mPosGBA.v[2],
                        (float)M.mnBAGlobalForKF};
    fwrite(v, sizeof(float), 9, o);
  }
  fclose(o);
  printf("GBA_SHIM_OK\n");
  return 0;
}
