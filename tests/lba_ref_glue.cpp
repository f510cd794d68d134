// lba_ref_glue.cpp — runs the reference's own Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1116-1498, copied at test time
// into tests/_build/lba_ref_body.inc, never committed) on a scene file against the stand-ins of tests/lba_ref_types.h.
//   usage: lba_ref <scene.bin> <out.bin>
// scene.bin is what tests/test_lba_shim.py's write_scene writes (tests/lba_shim_test.cpp describes it); all key frames live in ONE
// array, so the pointer-ordered observations maps are ordered by index.  out.bin begins with what tests/lba_shim_test.cpp writes
// for the drop-in (1, num_fixedKF, num_OptKF, num_edges, the change index, num_MPs; every key frame's pose and SetPose count; every
// point's position and its SetWorldPos / UpdateNormalAndDepth counts; the erase calls in order) and goes on with what the stand-in
// optimiser recorded: the vertices (id, kind, fixed, marginalized) and edges (type, both vertex ids) in the order added, the
// optimize() call and whether every erase call was made under the map's mutex.  TEST INFRASTRUCTURE.
#include <stdio.h>

#include "lba_ref_types.h"

namespace ORB_SLAM3 {
#include "lba_ref_body.inc"
}

namespace {
template <class T> T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "short scene file\n"); exit(2); } return v; }
}  // namespace

int main(int argc, char** argv) {
  using namespace ORB_SLAM3;
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int n_kf = rd<int>(f), n_mp = rd<int>(f), n_neigh = rd<int>(f), init_id = rd<int>(f), stop = rd<int>(f), inertial = rd<int>(f);
  static Map map, other;
  map.init_id = (long unsigned)init_id; map.inertial = inertial != 0;
  CallLog log;
  std::vector<KeyFrame> kfs((size_t)n_kf);   // ONE array: pointer order is index order
  std::vector<MapPoint> mps((size_t)n_mp);
  std::vector<std::vector<int>> feat_mp((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[(size_t)k];
    K.idx = k; K.log = &log; K.mpCamera = &K.cam;
    K.mnId = (long unsigned)rd<int>(f); K.bad = rd<int>(f) != 0; K.map = rd<int>(f) ? &other : &map;
    for (int i = 0; i < 4; ++i) K.pose.q.c[i] = rd<float>(f);
    for (int i = 0; i < 3; ++i) K.pose.t.v[i] = rd<float>(f);
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
  for (int p = 0; p < n_mp; ++p) {
    MapPoint& M = mps[(size_t)p];
    M.idx = p; M.mnId = (long unsigned)(1000 + 7 * p); M.log = &log;
    M.bad = rd<int>(f) != 0; M.map = rd<int>(f) ? &other : &map;
    for (int i = 0; i < 3; ++i) M.pos.v[i] = rd<float>(f);
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
  Optimizer::LocalBundleAdjustment(&kfs[0], &flag, &map, num_fixed, num_opt, num_mps, num_edges);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int head[6] = {1, num_fixed, num_opt, num_edges, map.change, num_mps};
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
  const g2o::SparseOptimizer::Record& R = g2o::SparseOptimizer::record();
  const int tail[8] = {(int)R.vertex.size(), (int)R.edge.size(), R.optimize_calls, R.max_iterations, R.ran, R.iterations, R.trials,
                       log.mutex_held_at_every_call ? 1 : 0};
  fwrite(tail, sizeof(int), 8, o);
  if (!R.vertex.empty()) fwrite(R.vertex.data(), sizeof(int), R.vertex.size(), o);
  if (!R.edge.empty()) fwrite(R.edge.data(), sizeof(int), R.edge.size(), o);
  const double dbl[3] = {R.user_lambda_init, R.delta[0], R.delta[1]};
  fwrite(dbl, sizeof(double), 3, o);
  fclose(o);
  printf("LBA_REF_OK fixed %d opt %d edges %d\n", num_fixed, num_opt, num_edges);
  return 0;
}
