// mlpnp_ref_glue.cpp — the reference's own MLPnPsolver constructor, iterate, SetRansacParameters, CheckInliers and Refine and
// Pinhole::project / unproject (cut out of the reference by signature into the build directory by tests/mlpnp_golden.py and
// compiled unmodified against tests/mlpnp_ref_types.h) on a case file, with the reference's DUtils::Random over rand() after
// srand(seed).  TEST INFRASTRUCTURE.
//   usage: mlpnp_ref <case.bin> <out.bin>
// case.bin: seed, the six arguments of SetRansacParameters (probability as float), the iterations per call, the number of
// calls at most, the calls to go on for after a success, n features, n_levels; then per feature state (1: a map point, 2: a bad one, 0: none), octave, xy, world
// position; K; sigma2.
// out.bin: mRansacMinInliers, mRansacMaxIts, N, the number of calls; per call of iterate(step, ...): the iterations it ran, the
// return value, bNoMore, nInliers, mnIterations and mnBestInliers after it, the sets it drew (ran x 6, as computePose received
// them), Tout, mBestTcw and vbInliers (n bytes; all 0 when the vector came back empty); then how often computePose was called
// with six points and with another number (Refine's calls).
#include <stdio.h>

// Compiled with -DMLPNP_SHIM the same program runs the drop-in rgbl_shim::MLPnPsolver<Frame, MapPoint> (shim/MLPnPsolver.h) on the
// stand-in Frame and MapPoint instead, against whichever library it is linked with, and writes the same file (the pose counts:
// the iterations run and -1): tests/test_mlpnp_shim.py compares it with the fixtures.  That build uses nothing of the reference:
// the camera's two virtual members (which the drop-in never calls) are stated here, and DUtils::Random::RandomInt is the
// stand-in of tests/sim3_shim_test.cpp: the reference's formula (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) over glibc's rand()
// generator with a state of the test's own (initstate_r / random_r give the numbers of srand(seed) / rand(); the process-wide
// stream is not the test's alone once a GPU runtime with threads of its own is loaded).  That it is right is not taken on
// trust: the sets drawn through it must be the ones the reference's own Random.cpp drew, recorded in tests/golden/mlpnp.
#ifdef MLPNP_SHIM
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
namespace test_rng {
static char table[128];
static struct random_data data;
static void seed(unsigned s) {
  memset(&data, 0, sizeof(data));
  initstate_r(s, table, sizeof(table), &data);
}
static int next() {
  int32_t v = 0;
  random_r(&data, &v);
  return (int)v;
}
}  // namespace test_rng
namespace DUtils {
struct Random {
  static int RandomInt(int min, int max) {
    int d = max - min + 1;
    return int(((double)test_rng::next() / ((double)RAND_MAX + 1.0)) * d) + min;
  }
};
}  // namespace DUtils
#define SEED(s) test_rng::seed((unsigned)(s))
#else
#define SEED(s) srand((unsigned)(s))
#endif

#include "mlpnp_ref_types.h"

#ifdef MLPNP_SHIM
#include "MLPnPsolver.h"
namespace ORB_SLAM3 {   // a pinhole camera; the drop-in reads GetType() and getParameter() only
cv::Point2f Pinhole::project(const cv::Point3f& X) {
  const float fx = mvParameters[0], fy = mvParameters[1], cx = mvParameters[2], cy = mvParameters[3];
  return cv::Point2f(cx + fx * (X.x / X.z), cy + fy * (X.y / X.z));
}
cv::Point3f Pinhole::unproject(const cv::Point2f& u) {
  const float fx = mvParameters[0], fy = mvParameters[1], cx = mvParameters[2], cy = mvParameters[3];
  return cv::Point3f((u.x - cx) / fx, (u.y - cy) / fy, 1.0f);
}
}  // namespace ORB_SLAM3
typedef rgbl_shim::MLPnPsolver<ORB_SLAM3::Frame, ORB_SLAM3::MapPoint> DropIn;
#else
#include "mlpnp_ref_bodies.inc"
#endif

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int32_t seed, min_inliers, max_its, min_set, step, max_calls, after_success, n, n_levels;
  float prob, epsilon, th2, K[4];
  CHECK(rd(f, &seed, 1) && rd(f, &prob, 1) && rd(f, &min_inliers, 1) && rd(f, &max_its, 1) && rd(f, &min_set, 1) && rd(f, &epsilon, 1) && rd(f, &th2, 1));
  CHECK(rd(f, &step, 1) && rd(f, &max_calls, 1) && rd(f, &after_success, 1) && rd(f, &n, 1) && rd(f, &n_levels, 1));
  std::vector<int32_t> state(n), oct(n);
  std::vector<float> xy(2 * (size_t)n), wp(3 * (size_t)n), sigma2(n_levels);
  CHECK(rd(f, state.data(), n) && rd(f, oct.data(), n) && rd(f, xy.data(), 2 * (size_t)n) && rd(f, wp.data(), 3 * (size_t)n) && rd(f, K, 4) && rd(f, sigma2.data(), n_levels));
  fclose(f);
  ORB_SLAM3::Pinhole cam;
  cam.mvParameters.assign(K, K + 4);
  ORB_SLAM3::Frame F;
  F.mpCamera = &cam;
  F.mvLevelSigma2 = sigma2;
  F.mvKeysUn.resize(n);
  F.mvpMapPoints.assign(n, nullptr);
  std::vector<ORB_SLAM3::MapPoint> points(n);
  std::vector<ORB_SLAM3::MapPoint*> matches(n, nullptr);
  for (int i = 0; i < n; ++i) {
    F.mvKeysUn[i].pt = cv::Point2f(xy[2 * i], xy[2 * i + 1]);
    F.mvKeysUn[i].octave = oct[i];
    points[i].pos = Eigen::Vector3f(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]);
    points[i].bad = state[i] == 2;
    if (state[i]) matches[i] = &points[i];
  }
  SEED(seed);
#ifdef MLPNP_SHIM
  DropIn solver(F, matches);
  solver.SetRansacParameters((double)prob, min_inliers, max_its, min_set, epsilon, th2);
  auto iterations = [&]() { return solver.GetIterations(); };
  auto best = [&]() { return solver.GetBestInliers(); };
#else
  ORB_SLAM3::MLPnPsolver solver(F, matches);
  solver.SetRansacParameters((double)prob, min_inliers, max_its, min_set, epsilon, th2);
  auto iterations = [&]() { return solver.mnIterations; };
  auto best = [&]() { return solver.mnBestInliers; };
#endif
  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  std::vector<uint8_t> body;
  auto put = [&](const void* p, size_t bytes) { body.insert(body.end(), (const uint8_t*)p, (const uint8_t*)p + bytes); };
  int32_t calls = 0;
  for (; calls < max_calls; ++calls) {
    const int before = iterations();
#ifndef MLPNP_SHIM
    const int poses_before = solver.compute_pose_calls;
#endif
    bool no_more = false;
    std::vector<bool> inl;
    int n_inl = 0;
    Eigen::Matrix4f T;
    const bool ret = solver.iterate(step, no_more, inl, n_inl, T);
    const int32_t ran = iterations() - before;
    const int32_t head[6] = {ran, ret ? 1 : 0, no_more ? 1 : 0, n_inl, iterations(), best()};
    put(head, sizeof(head));
#ifdef MLPNP_SHIM
    put(solver.LastSamples().data(), 24 * (size_t)ran);   // the sets the scan reached, of those drawn
    put(T.d, 64);
    put(solver.GetBestTcw(), 64);
#else
    CHECK(solver.compute_pose_calls - poses_before == ran);
    put(solver.drawn.data() + 6 * (size_t)(solver.drawn.size() / 6 - ran), 24 * (size_t)ran);
    put(T.d, 64);
    put(solver.mBestTcw.d, 64);
#endif
    std::vector<uint8_t> fl(n, 0);
    for (int i = 0; i < n && i < (int)inl.size(); ++i) fl[i] = inl[i] ? 1 : 0;
    put(fl.data(), n);
    if (no_more || (ret && after_success-- <= 0)) { ++calls; break; }
  }
#ifdef MLPNP_SHIM
  {   // IterateBatch: two fresh solvers after the same seed; the first draws first, so its call is the first call above
    SEED(seed);
    DropIn a(F, matches), b(F, matches);
    a.SetRansacParameters((double)prob, min_inliers, max_its, min_set, epsilon, th2);
    b.SetRansacParameters((double)prob, min_inliers, max_its, min_set, epsilon, th2);
    std::vector<char> no_more, found;
    std::vector<std::vector<bool> > inl;
    std::vector<int> n_inl;
    std::vector<Eigen::Matrix4f> T;
    CHECK(DropIn::IterateBatch(std::vector<DropIn*>{&a, &b}, step, no_more, inl, n_inl, T, found));
    CHECK(found.size() == 2 && body.size() >= 24);
    int32_t head[6];
    memcpy(head, body.data(), sizeof(head));
    CHECK(found[0] == head[1] && no_more[0] == head[2] && n_inl[0] == head[3] && a.GetIterations() == head[4] && a.GetBestInliers() == head[5]);
    CHECK(memcmp(T[0].d, body.data() + 24 + 24 * (size_t)head[0], 64) == 0);
    CHECK((int)inl[1].size() == (found[1] ? n : 0) && (solver.GetN() >= solver.GetMinInliers() ? b.GetIterations() > 0 : b.GetIterations() == 0));
    // solvers of different devices in one batch are refused: nothing runs, every solver reports bNoMore
    DropIn c(F, matches, 0), d(F, matches, 1);
    CHECK(!DropIn::IterateBatch(std::vector<DropIn*>{&c, &d}, step, no_more, inl, n_inl, T, found));
    CHECK(found[0] == 0 && found[1] == 0 && no_more[0] == 1 && no_more[1] == 1 && c.GetIterations() == 0 && d.GetIterations() == 0);
  }
  {   // the two refusals: a camera that is not a Pinhole, and a minimal set other than six
    ORB_SLAM3::Pinhole fisheye;
    fisheye.mvParameters.assign(K, K + 4);
    fisheye.type = 1;   // GeometricCamera::CAM_FISHEYE
    ORB_SLAM3::Frame G = F;
    G.mpCamera = &fisheye;
    DropIn refused(G, matches), sets_of_four(F, matches);
    refused.SetRansacParameters((double)prob, min_inliers, max_its, min_set, epsilon, th2);
    sets_of_four.SetRansacParameters((double)prob, min_inliers, max_its, 4, epsilon, th2);
    DropIn* both[2] = {&refused, &sets_of_four};
    for (DropIn* s : both) {
      bool no_more = false;
      std::vector<bool> inl(3, true);
      int n_inl = 7;
      Eigen::Matrix4f T;
      CHECK(!s->iterate(step, no_more, inl, n_inl, T) && no_more && inl.empty() && n_inl == 0 && s->GetIterations() == 0);
      CHECK(T(0, 0) == 1.0f && T(0, 1) == 0.0f && T(3, 3) == 1.0f);
    }
  }
  const int32_t top[4] = {solver.GetMinInliers(), solver.GetMaxIterations(), solver.GetN(), calls};
  const int32_t tail[2] = {iterations(), -1};
#else
  const int32_t top[4] = {solver.mRansacMinInliers, solver.mRansacMaxIts, solver.N, calls};
  const int32_t tail[2] = {solver.compute_pose_calls, solver.refine_pose_calls};
#endif
  fwrite(top, 4, 4, o);
  fwrite(body.data(), 1, body.size(), o);
  fwrite(tail, 4, 2, o);
  fclose(o);
  printf("MLPNP_REF_OK\n");
  return 0;
}
