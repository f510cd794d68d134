// sim3_ref_glue.cpp — the reference's own Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc, copied without their #include
// lines into the build directory by tests/sim3_golden.py and compiled unmodified against tests/sim3_ref_types.h) on a case file
// of tests/sim3_shim_test.cpp's format, with the reference's DUtils::Random over rand() after srand(seed).  TEST INFRASTRUCTURE.
//   usage: sim3_ref <case.bin> <out.bin>
// out.bin: mRansacMaxIts, N, the number of calls; then for every call of iterate(20, ...) of the SECOND overload, until bNoMore
// or bConverge: the iterations it ran, bNoMore, bConverge, nInliers, mnIterations and mnBestInliers after it, the triples it
// drew (the indices of the elements of mvX3Dc1 it copied into P3Dc1i), the matrix returned, GetEstimatedTransformation() and
// vbInliers; then the same walk with the FIRST overload on a fresh solver after the same srand: the number of calls, and per
// call bNoMore, nInliers, the matrix returned and vbInliers.
#include <stdio.h>
#include <string.h>

#include "sim3_ref_types.h"

#include "sim3_ref_bodies.inc"

namespace {
using ORB_SLAM3::KeyFrame;
using ORB_SLAM3::MapPoint;

struct Probe : ORB_SLAM3::Sim3Solver {
  using ORB_SLAM3::Sim3Solver::Sim3Solver;
  const Eigen::Vector3f* first() const { return mvX3Dc1.data(); }
  int count() const { return (int)mvX3Dc1.size(); }
  int iterations() const { return mnIterations; }
  int best() const { return mnBestInliers; }
  int max_its() const { return mRansacMaxIts; }
  int n() const { return N; }
};
const Eigen::Vector3f* g_first = nullptr;
int g_count = 0;
std::vector<int32_t> g_drawn;
void on_column(const Eigen::Vector3f* p) {
  if (g_first && p >= g_first && p < g_first + g_count) g_drawn.push_back((int32_t)(p - g_first));
}

template <class T> bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

void put_flags(FILE* o, const std::vector<bool>& flags, int n1) {
  std::vector<uint8_t> fl(n1, 0);
  for (int i = 0; i < n1 && i < (int)flags.size(); ++i) fl[i] = flags[i] ? 1 : 0;
  fwrite(fl.data(), 1, n1, o);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  int seed = 0, min_inliers = 0, fix_scale = 0, n1 = 0, n_levels = 0;
  CHECK(rd(f, &seed, 1) && rd(f, &min_inliers, 1) && rd(f, &fix_scale, 1) && rd(f, &n1, 1) && rd(f, &n_levels, 1));
  std::vector<int32_t> state(n1), oct1(n1), oct2(n1);
  std::vector<float> xw1(3 * (size_t)n1), xw2(3 * (size_t)n1), sigma2(n_levels);
  float K[4];
  ORB_SLAM3::Pinhole pinhole;
  KeyFrame kf1, kf2;
  CHECK(rd(f, state.data(), n1) && rd(f, oct1.data(), n1) && rd(f, oct2.data(), n1) && rd(f, xw1.data(), 3 * (size_t)n1) && rd(f, xw2.data(), 3 * (size_t)n1));
  CHECK(rd(f, kf1.R.m, 9) && rd(f, kf1.t.v, 3) && rd(f, kf2.R.m, 9) && rd(f, kf2.t.v, 3) && rd(f, K, 4) && rd(f, sigma2.data(), n_levels));
  fclose(f);
  pinhole.mvParameters.assign(K, K + 4);

  // key frame 1 observes point i at feature i; key frame 2 observes its match at feature n1 - 1 - i (as sim3_shim_test.cpp)
  std::vector<MapPoint> p1(n1), p2(n1);
  std::vector<MapPoint*> matched(n1, nullptr);
  kf1.mpCamera = kf2.mpCamera = &pinhole;
  kf1.mvLevelSigma2 = kf2.mvLevelSigma2 = sigma2;
  kf1.mvpMapPoints.assign(n1, nullptr);
  kf1.mvKeysUn.resize(n1); kf2.mvKeysUn.resize(n1);
  for (int i = 0; i < n1; ++i) {
    for (int c = 0; c < 3; ++c) { p1[i].pos.v[c] = xw1[3 * i + c]; p2[i].pos.v[c] = xw2[3 * i + c]; }
    p1[i].kf = &kf1; p1[i].index = i;
    p2[i].kf = &kf2; p2[i].index = n1 - 1 - i;
    kf1.mvKeysUn[i].octave = oct1[i];
    kf2.mvKeysUn[n1 - 1 - i].octave = oct2[i];
    if (state[i] != 0) matched[i] = &p2[i];
    if (state[i] != 1) kf1.mvpMapPoints[i] = &p1[i];
    if (state[i] == 2) (i % 2 ? p1[i] : p2[i]).bad = true;
    if (state[i] == 3) (i % 2 ? p1[i] : p2[i]).index = -1;
  }

  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  Eigen::sim3_ref_on_column = on_column;
  {
    srand((unsigned)seed);
    Probe s(&kf1, &kf2, matched, fix_scale != 0);
    s.SetRansacParameters(0.99, min_inliers, 300);
    g_first = s.first(); g_count = s.count();
    struct Rec { int head[6]; std::vector<int32_t> drawn; Eigen::Matrix4f T, best; std::vector<bool> flags; };
    std::vector<Rec> recs;
    for (int k = 0; k < 64; ++k) {
      Rec r;
      bool no_more = false, converge = false;
      int inliers = 0;
      const int before = s.iterations();
      g_drawn.clear();
      r.T = s.iterate(20, no_more, r.flags, inliers, converge);
      r.best = s.GetEstimatedTransformation();
      r.drawn = g_drawn;
      const int ran = s.iterations() - before;
      CHECK((int)r.drawn.size() == 3 * ran);
      const int head[6] = {ran, no_more ? 1 : 0, converge ? 1 : 0, inliers, s.iterations(), s.best()};
      memcpy(r.head, head, sizeof(head));
      recs.push_back(r);
      if (no_more || converge) break;
    }
    CHECK(recs.back().head[1] || recs.back().head[2]);
    const int head[3] = {s.max_its(), s.n(), (int)recs.size()};
    fwrite(head, sizeof(int), 3, o);
    for (const Rec& r : recs) {
      fwrite(r.head, sizeof(int), 6, o);
      fwrite(r.drawn.data(), sizeof(int32_t), r.drawn.size(), o);
      fwrite(r.T.m, sizeof(float), 16, o);
      fwrite(r.best.m, sizeof(float), 16, o);
      put_flags(o, r.flags, n1);
    }
    g_first = nullptr;
  }
  {
    srand((unsigned)seed);
    Probe s(&kf1, &kf2, matched, fix_scale != 0);
    s.SetRansacParameters(0.99, min_inliers, 300);
    std::vector<int> heads;
    std::vector<Eigen::Matrix4f> Ts;
    std::vector<std::vector<bool> > flags;
    for (int k = 0; k < 64; ++k) {
      bool no_more = false;
      int inliers = 0;
      std::vector<bool> fl;
      Ts.push_back(s.iterate(20, no_more, fl, inliers));
      flags.push_back(fl);
      heads.push_back(no_more ? 1 : 0);
      heads.push_back(inliers);
      if (no_more || inliers > 0) break;   // the first overload reports convergence through nInliers alone
    }
    const int calls = (int)Ts.size();
    fwrite(&calls, sizeof(int), 1, o);
    for (int k = 0; k < calls; ++k) {
      fwrite(&heads[2 * k], sizeof(int), 2, o);
      fwrite(Ts[k].m, sizeof(float), 16, o);
      put_flags(o, flags[k], n1);
    }
  }
  fclose(o);
  printf("SIM3_REF_OK\n");
  return 0;
}
