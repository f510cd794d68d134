// lba_shim_test.cpp — the drop-in rgbl_shim::LocalBundleAdjustment (orb_slam3_rgbl_amd/shim/LocalBundleAdjuster.h) on stand-in
// KeyFrame / MapPoint / Map types of its own.
//   usage: lba_shim_test <scene.bin> <out.bin> [localmap]
// With `localmap` the drop-in gets a stand-in device local map that records its Refresh calls; out.bin then ends with the number
// of Refresh calls, the points of the last one, its two flags and whether they were the local points in order.
// scene.bin (tests/test_lba_shim.py writes it): n_kf, n_mp, n_neigh, init_id, stop, inertial; per key frame id, bad, other_map,
// q (x y z w), t, K, bf, n_features and per feature x, y, octave, uright, map point (-1: none); per map point bad, other_map, pos;
// the covisible list of key frame 0 (indices); n_extra and that many (key frame, map point) observations whose left index is -1;
// the 8 entries of mvInvLevelSigma2.  All key frames live in ONE array, so the
// pointer-ordered observations maps are ordered by index.  out.bin: the drop-in's return value, num_fixedKF, num_OptKF,
// num_edges, the change index, every key frame's pose and SetPose count, every point's position and its SetWorldPos /
// UpdateNormalAndDepth counts, then the erase calls in the order they were made.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/LocalBundleAdjuster.h"

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
struct Map {
  long unsigned init_id = 0;
  bool inertial = false;
  int change = 0;
  std::mutex mMutexMapUpdate;
  long unsigned GetInitKFid() { return init_id; }
  bool IsInertial() { return inertial; }
  void IncreaseChangeIndex() { ++change; }
};
struct KeyFrame;
struct EraseLog { std::vector<int> calls; };   // 0 kf mp: EraseMapPointMatch, 1 kf mp: EraseObservation
struct MapPoint {
  int idx = 0;
  V3 pos;
  bool bad = false;
  Map* map = nullptr;
  long unsigned mnBALocalForKF = 0;
  std::map<KeyFrame*, std::tuple<int, int>> obs;
  int set_pos = 0, updated = 0;
  EraseLog* log = nullptr;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  V3 GetWorldPos() { return pos; }
  void SetWorldPos(const V3& p) { pos = p; ++set_pos; }
  void UpdateNormalAndDepth() { ++updated; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return obs; }
  void EraseObservation(KeyFrame* kf);
};
struct KeyFrame {
  int idx = 0;
  long unsigned mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  bool bad = false;
  Map* map = nullptr;
  SE3 pose;
  int set_pose = 0;
  Camera cam;
  Camera* mpCamera = &cam;
  Camera* mpCamera2 = nullptr;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> covisible;
  EraseLog* log = nullptr;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  SE3 GetPose() { return pose; }
  void SetPose(const SE3& T) { pose = T; ++set_pose; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covisible; }
  std::vector<MapPoint*> GetMapPointMatches() { return mps; }
  void EraseMapPointMatch(MapPoint* mp) { log->calls.push_back(0); log->calls.push_back(idx); log->calls.push_back(mp->idx); }
};
void MapPoint::EraseObservation(KeyFrame* kf) { log->calls.push_back(1); log->calls.push_back(kf->idx); log->calls.push_back(idx); }

struct LocalMap {   // what the drop-in needs of rgbl_shim::DeviceLocalMap
  int calls = 0, points = 0, normal = -1, descriptor = -1;
  std::vector<MapPoint*> last;
  bool Refresh(const std::vector<MapPoint*>& v, bool n, bool d) { ++calls; points = (int)v.size(); normal = n; descriptor = d; last = v; return true; }
};

template <class T> T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short scene file\n"); exit(2); } return v; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int n_kf = rd<int>(f), n_mp = rd<int>(f), n_neigh = rd<int>(f), init_id = rd<int>(f), stop = rd<int>(f), inertial = rd<int>(f);
  Map map, other;
  map.init_id = (long unsigned)init_id; map.inertial = inertial != 0;
  EraseLog log;
  std::vector<KeyFrame> kfs((size_t)n_kf);   // ONE array: pointer order is index order
  std::vector<MapPoint> mps((size_t)n_mp);
  std::vector<std::vector<int>> feat_mp((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[(size_t)k];
    K.idx = k; K.log = &log;
    K.mnId = (long unsigned)rd<int>(f); K.bad = rd<int>(f) != 0; K.map = rd<int>(f) ? &other : &map;
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
  for (int p = 0; p < n_mp; ++p) {
    MapPoint& M = mps[(size_t)p];
    M.idx = p; M.log = &log;
    M.bad = rd<int>(f) != 0; M.map = rd<int>(f) ? &other : &map;
    const float x = rd<float>(f), y = rd<float>(f), z = rd<float>(f);
    M.pos = V3(x, y, z);
  }
  for (int i = 0; i < n_neigh; ++i) kfs[0].covisible.push_back(&kfs[(size_t)rd<int>(f)]);
  const int n_extra = rd<int>(f);
  std::vector<std::pair<int, int>> extra;
  for (int i = 0; i < n_extra; ++i) { const int k = rd<int>(f), p = rd<int>(f); extra.push_back(std::make_pair(k, p)); }
  std::vector<float> sigma;
  for (int i = 0; i < 8; ++i) sigma.push_back(rd<float>(f));
  fclose(f);
  for (int k = 0; k < n_kf; ++k) {
    kfs[(size_t)k].mvInvLevelSigma2 = sigma;
    for (size_t i = 0; i < feat_mp[(size_t)k].size(); ++i) {
      const int p = feat_mp[(size_t)k][i];
      kfs[(size_t)k].mps.push_back(p >= 0 ? &mps[(size_t)p] : nullptr);
      if (p >= 0) mps[(size_t)p].obs[&kfs[(size_t)k]] = std::make_tuple((int)i, -1);
    }
  }
  for (auto& e : extra) mps[(size_t)e.second].obs[&kfs[(size_t)e.first]] = std::make_tuple(-1, 0);
  bool flag = stop != 0;
  int num_fixed = -7, num_opt = -7, num_mps = -7, num_edges = -7;
  const bool with_local_map = argc > 3;
  LocalMap local_map;
  const bool done = with_local_map ? rgbl_shim::LocalBundleAdjustment(&kfs[0], &flag, &map, num_fixed, num_opt, num_mps, num_edges, &local_map)
                                   : rgbl_shim::LocalBundleAdjustment(&kfs[0], &flag, &map, num_fixed, num_opt, num_mps, num_edges);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int head[6] = {done ? 1 : 0, num_fixed, num_opt, num_edges, map.change, num_mps};
  fwrite(head, sizeof(int), 6, o);
  for (KeyFrame& K : kfs) {
    const float v[8] = {K.pose.q.c[0], K.pose.q.c[1], K.pose.q.c[2], K.pose.q.c[3], K.pose.t.v[0], K.pose.t.v[1], K.pose.t.v[2], (float)K.set_pose};
    fwrite(v, sizeof(float), 8, o);
  }
  for (MapPoint& M : mps) {
    const float v[5] = {M.pos.v[0], M.pos.v[1], M.pos.v[2], (float)M.set_pos, (float)M.updated};
    fwrite(v, sizeof(float), 5, o);
  }
  const int n_calls = (int)log.calls.size();
  fwrite(&n_calls, sizeof(int), 1, o);
  if (n_calls) fwrite(log.calls.data(), sizeof(int), (size_t)n_calls, o);
  if (with_local_map) {
    int in_order = 1;
    size_t j = 0;
    for (MapPoint& M : mps)   // the moved points are exactly the ones SetWorldPos was called on
      if (M.set_pos && !(j < local_map.last.size())) in_order = 0; else if (M.set_pos) ++j;
    for (MapPoint* p : local_map.last) if (!p->set_pos) in_order = 0;
    const int tail[5] = {local_map.calls, local_map.points, local_map.normal, local_map.descriptor, in_order && j == local_map.last.size() ? 1 : 0};
    fwrite(tail, sizeof(int), 5, o);
  }
  fclose(o);
  printf("LBA_SHIM_OK\n");
  return 0;
}
