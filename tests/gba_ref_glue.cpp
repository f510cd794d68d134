// gba_ref_glue.cpp — runs the reference's own Optimizer::BundleAdjustment (src/Optimizer.cc:60-390, copied at test time into
// tests/_build/gba_ref_body.inc, never committed) on a scene file against the stand-ins of tests/gba_ref_types.h.
//   usage: gba_ref <scene.bin> <out.bin>
// scene.bin is what tests/test_gba_shim.py's write_scene writes (tests/gba_shim_test.cpp describes it); all key frames live in
// ONE array, so the pointer-ordered observations maps are ordered by index.  out.bin begins with what tests/gba_shim_test.cpp
// writes for the drop-in (1; per key frame its pose, SetPose count, mTcwGBA, mnBAGlobalForKF; per map point its position,
// SetWorldPos and UpdateNormalAndDepth counts, mPosGBA, mnBAGlobalForKF) and goes on with what the stand-in optimiser recorded:
// the vertices (id, kind, fixed, marginalized) and edges (type, both vertex ids) in the order added, the ids handed to
// removeVertex, the optimize() call, whether the edges had a kernel, and both Huber deltas.  TEST INFRASTRUCTURE.
#include <stdio.h>

#include "gba_ref_types.h"

namespace ORB_SLAM3 {
#include "gba_ref_body.inc"
}

namespace {
template <class T> T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short scene file\n"); exit(2); } return v; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int n_kf = rd<int>(f), n_mp = rd<int>(f), init_id = rd<int>(f), origin = rd<int>(f), stop = rd<int>(f), loop_kf = rd<int>(f),
            robust = rd<int>(f), iterations = rd<int>(f), through_map = rd<int>(f);
  using namespace ORB_SLAM3;
  static Map map;
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
    for (int i = 0; i < 4; ++i) K.pose.q.c[i] = q[i];
    for (int i = 0; i < 3; ++i) K.pose.t.v[i] = t[i];
    for (int i = 0; i < 4; ++i) K.cam.K[i] = rd<float>(f);
    K.fx = K.cam.K[0]; K.fy = K.cam.K[1]; K.cx = K.cam.K[2]; K.cy = K.cam.K[3];
    K.mbf = rd<float>(f);
    const int nf = rd<int>(f);
    for (int i = 0; i < nf; ++i) {
      cv::KeyPoint kp; kp.pt.x = rd<float>(f); kp.pt.y = rd<float>(f); kp.octave = rd<int>(f);
      K.mvKeysUn.push_back(kp); K.mvuRight.push_back(rd<float>(f));
      feat_mp[(size_t)k].push_back(rd<int>(f));
    }
  }
  map.origin = &kfs[(size_t)origin];
  for (int p = 0; p < n_mp; ++p) {
    MapPoint& M = mps[(size_t)p];
    M.mnId = (long unsigned)rd<int>(f); M.bad = rd<int>(f) != 0;
    const float x = rd<float>(f), y = rd<float>(f), z = rd<float>(f);
    M.pos.v[0] = x; M.pos.v[1] = y; M.pos.v[2] = z;
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
  (void)through_map;   // :52-57 only gathers the two vectors
  bool flag = stop != 0;
  Optimizer::BundleAdjustment(vpKFs, vpMP, iterations, &flag, (unsigned long)loop_kf, robust != 0);
  const bool done = true;
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
  const g2o::SparseOptimizer::Record& R = g2o::SparseOptimizer::record();
  const int tail[9] = {(int)R.vertex.size(), (int)R.edge.size(), (int)R.removed.size(), R.optimize_calls, R.max_iterations, R.iterations, R.trials,
                       R.robust, R.polls};
  fwrite(tail, sizeof(int), 9, o);
  if (!R.vertex.empty()) fwrite(R.vertex.data(), sizeof(int), R.vertex.size(), o);
  if (!R.edge.empty()) fwrite(R.edge.data(), sizeof(int), R.edge.size(), o);
  if (!R.removed.empty()) fwrite(R.removed.data(), sizeof(int), R.removed.size(), o);
  fwrite(R.delta, sizeof(double), 2, o);
  fclose(o);
  printf("GBA_REF_OK\n");
  return 0;
}
