// sim3_opt_ref_glue.cpp — runs the reference's own Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381, copied at test time into
// tests/_build/sim3_opt_ref_body.inc, never committed) on a case file against the stand-ins of tests/sim3_opt_ref_types.h.
//   usage: sim3_opt_ref <case.bin> <out.bin>
// case.bin is what tests/test_sim3_opt_shim.py's write_case writes.  out.bin: the return value, the number of edge pairs, the
// optimize() calls (iterations asked for, pairs in the graph, edges with a kernel, iterations run), g2oS12 and the largest entry of
// mAcumHessian afterwards, which matches are null afterwards, and per pair its feature, obs2 and the information of e21.
// TEST INFRASTRUCTURE.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sim3_opt_ref_types.h"

namespace ORB_SLAM3 {
#include "sim3_opt_ref_body.inc"
}

namespace {
template <class T> std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  using namespace ORB_SLAM3;
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> hd = take<int32_t>(f, 6);
  const int n = hd[0], n2 = hd[1], np = hd[2], nl = hd[3];
  const bool fix_scale = hd[4] != 0, all_points = hd[5] != 0;
  const float th2 = take<float>(f, 1)[0];
  const auto mp1 = take<int32_t>(f, n), mt = take<int32_t>(f, n), i2 = take<int32_t>(f, n), lv2 = take<int32_t>(f, n);
  const auto bad = take<uint8_t>(f, np);
  const auto pos = take<float>(f, 3 * (size_t)np);
  const auto R1 = take<float>(f, 9), t1 = take<float>(f, 3), R2 = take<float>(f, 9), t2 = take<float>(f, 3);
  const auto xy1 = take<float>(f, 2 * (size_t)n); const auto oc1 = take<int32_t>(f, n);
  const auto xy2 = take<float>(f, 2 * (size_t)n2); const auto oc2 = take<int32_t>(f, n2);
  const auto sg1 = take<float>(f, nl), sg2 = take<float>(f, nl);
  const auto K1 = take<float>(f, 4), K2 = take<float>(f, 4);
  const auto est = take<double>(f, 8);
  fclose(f);

  GeometricCamera cam1, cam2;
  memcpy(cam1.K, K1.data(), 16); memcpy(cam2.K, K2.data(), 16);
  KeyFrame kf1, kf2;
  kf1.mpCamera = &cam1; kf2.mpCamera = &cam2;
  memcpy(kf1.R.m, R1.data(), 36); memcpy(kf1.t.v, t1.data(), 12); memcpy(kf2.R.m, R2.data(), 36); memcpy(kf2.t.v, t2.data(), 12);
  for (int i = 0; i < n; ++i) { cv::KeyPoint k(cv::Point2f(xy1[2 * i], xy1[2 * i + 1]), 31.0f, -1, 0, oc1[i]); kf1.mvKeysUn.push_back(k); }
  for (int i = 0; i < n2; ++i) { cv::KeyPoint k(cv::Point2f(xy2[2 * i], xy2[2 * i + 1]), 31.0f, -1, 0, oc2[i]); kf2.mvKeysUn.push_back(k); }
  kf1.mvInvLevelSigma2 = sg1; kf2.mvInvLevelSigma2 = sg2;
  std::vector<MapPoint> points((size_t)np);
  for (int p = 0; p < np; ++p) { memcpy(points[p].pos.v, &pos[3 * (size_t)p], 12); points[p].bad = bad[p] != 0; }
  kf1.mps.assign((size_t)n, nullptr);
  std::vector<MapPoint*> matches((size_t)n, nullptr);
  for (int i = 0; i < n; ++i) {
    if (mp1[i] >= 0) kf1.mps[i] = &points[mp1[i]];
    if (mt[i] >= 0) {
      MapPoint* m = &points[mt[i]];
      matches[i] = m;
      m->mnTrackScaleLevel = lv2[i];   // -1 where the case says so: the reference never uses it as an index
      m->seen_in = &kf2; m->index_there = i2[i];
    }
  }
  g2o::Sim3 S;
  memcpy(S.S.q, est.data(), 32); memcpy(S.S.t, est.data() + 4, 24); S.S.s = est[7];
  Eigen::Matrix<double, 7, 7> H;
  const int32_t r = Optimizer::OptimizeSim3(&kf1, &kf2, matches, S, th2, fix_scale, H, all_points);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const auto& edges = g2o::SparseOptimizer::all_edges();
  const auto& calls = g2o::SparseOptimizer::calls();
  const int32_t pairs = (int32_t)(edges.size() / 2), n_calls = (int32_t)calls.size();
  const double hmax = H.largest();
  fwrite(&r, 4, 1, o); fwrite(&pairs, 4, 1, o); fwrite(&n_calls, 4, 1, o);
  for (const auto& c : calls) fwrite(&c, sizeof(c), 1, o);
  fwrite(S.S.q, 8, 4, o); fwrite(S.S.t, 8, 3, o); fwrite(&S.S.s, 8, 1, o); fwrite(&hmax, 8, 1, o);
  for (int i = 0; i < n; ++i) { const uint8_t null_now = matches[i] == nullptr ? 1 : 0; fwrite(&null_now, 1, 1, o); }
  for (int k = 0; k < pairs; ++k) {
    const Sim3Edge* b = edges[2 * k + 1];
    const float rec[3] = {(float)b->obs.v[0], (float)b->obs.v[1], (float)b->info.d};
    fwrite(rec, 4, 3, o);
  }
  fclose(o);
  printf("SIM3_OPT_REF_OK result %d pairs %d optimize calls %d\n", r, pairs, n_calls);
  return 0;
}
