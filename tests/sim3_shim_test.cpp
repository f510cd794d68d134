// sim3_shim_test.cpp — the drop-in rgbl_shim::Sim3Solver (orb_slam3_rgbl_amd/shim/Sim3Solver.h) on stand-in KeyFrame / MapPoint /
// matrix types of its own.
//   usage: sim3_shim_test <case.bin> <out.bin>
// case.bin (tests/test_sim3_shim.py writes it): seed, min_inliers, fix_scale, n1, n_levels, then per feature of key frame 1:
// state (0 no match, 1 no map point in key frame 1, 2 a bad point, 3 no index in its key frame, 4 a correspondence), octave1,
// octave2, Xw1, Xw2; then Rcw1, tcw1, Rcw2, tcw2, K, mvLevelSigma2.
// out.bin: mRansacMaxIts, N, the number of calls and of rand() values they used, then for every call of iterate(20, ...) (second overload, until bNoMore or bConverge): the number of
// triples drawn, the triples, bNoMore, bConverge, nInliers, mnIterations and mnBestInliers after the call, the matrix returned
// and vbInliers.  The Python side compares them with what the reference's own code recorded (tests/golden/sim3) and replays them
// through rgbl_sim3_ransac_host.
// Checked here: the first overload and find against the second; SolveBatch against single solvers; a DeviceLocalMap against host
// arrays; N < mRansacMinInliers; a call after the iterations are used up; a fisheye camera (refused).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/ORBmatcher.h"

// The stand-in is DUtils::Random::RandomInt's formula (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) over glibc's rand() generator
// with a state of the test's own (initstate_r / random_r: the numbers of srand(seed) / rand()): the process-wide stream is not
// the test's alone once a GPU runtime with threads of its own is loaded.  That both are right is not taken on trust: the triples
// drawn through them must be the ones the reference's own Random.cpp drew after srand(seed), recorded in tests/golden/sim3.
namespace test_rng {
static char table[128];
static struct random_data data;
static long draws = 0;
static void seed(unsigned s) {
  memset(&data, 0, sizeof(data));
  initstate_r(s, table, sizeof(table), &data);
  draws = 0;
}
static int next() {
  int32_t v = 0;
  random_r(&data, &v);
  ++draws;
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

#include "../orb_slam3_rgbl_amd/shim/Sim3Solver.h"

namespace {

struct V3 {
  float v[3] = {0, 0, 0};
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
};
struct M3 {
  float m[9] = {0};
  float& operator()(int i, int j) { return m[3 * i + j]; }
  float operator()(int i, int j) const { return m[3 * i + j]; }
};
struct M4 {
  float m[16] = {0};
  float& operator()(int i, int j) { return m[4 * i + j]; }
  float operator()(int i, int j) const { return m[4 * i + j]; }
};
struct Camera {
  unsigned type = 0;   // GeometricCamera::CAM_PINHOLE
  float K[4] = {0, 0, 0, 0};
  unsigned GetType() const { return type; }
  float getParameter(int i) const { return K[i]; }
};
struct KeyFrame;
struct MapPoint {
  static std::mutex mGlobalMutex;
  V3 pos;
  bool bad = false;
  KeyFrame* kf = nullptr;   // the key frame that observes it ...
  int index = -1;           // ... at this feature
  bool isBad() const { return bad; }
  std::tuple<int, int> GetIndexInKeyFrame(KeyFrame* p) const { return p == kf ? std::make_tuple(index, -1) : std::make_tuple(-1, -1); }
  V3 GetWorldPos() { return pos; }
  V3 GetNormal() { V3 n; n.v[2] = 1; return n; }
  float GetMinDistance() { return 1.0f; }
  float GetMaxDistance() { return 100.0f; }
  cv::Mat GetDescriptor() { return cv::Mat::zeros(1, 32, CV_8U); }
};
std::mutex MapPoint::mGlobalMutex;
struct KeyFrame {
  Camera* mpCamera = nullptr;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvLevelSigma2;
  M3 R; V3 t;
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  M3 GetRotation() { return R; }
  V3 GetTranslation() { return t; }
};
typedef rgbl_shim::Sim3Solver<KeyFrame, M4> Solver;

template <class T> bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

bool same(const M4& a, const M4& b) {
  for (int i = 0; i < 16; ++i)
    if (!(a.m[i] == b.m[i] || (a.m[i] != a.m[i] && b.m[i] != b.m[i]))) return false;
  return true;
}
bool identity(const M4& a) {
  for (int i = 0; i < 16; ++i)
    if (a.m[i] != (i % 5 == 0 ? 1.0f : 0.0f)) return false;
  return true;
}
struct CallRecord {
  bool no_more = false, converge = false;
  int inliers = 0, iterations = 0, best = 0;
  M4 T;
  std::vector<bool> flags;
  std::vector<int32_t> samples;
};
// iterate(step, ...) of the second overload until bNoMore or bConverge
std::vector<CallRecord> run_all(Solver& s, int step) {
  std::vector<CallRecord> out;
  for (int k = 0; k < 64; ++k) {
    CallRecord r;
    r.T = s.iterate(step, r.no_more, r.flags, r.inliers, r.converge);
    r.iterations = s.GetIterations(); r.best = s.GetBestInliers(); r.samples = s.GetLastSamples();
    out.push_back(r);
    if (r.no_more || r.converge) break;
  }
  return out;
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
  Camera pinhole, fisheye;
  KeyFrame kf1, kf2;
  CHECK(rd(f, state.data(), n1) && rd(f, oct1.data(), n1) && rd(f, oct2.data(), n1) && rd(f, xw1.data(), 3 * (size_t)n1) && rd(f, xw2.data(), 3 * (size_t)n1));
  CHECK(rd(f, kf1.R.m, 9) && rd(f, kf1.t.v, 3) && rd(f, kf2.R.m, 9) && rd(f, kf2.t.v, 3) && rd(f, pinhole.K, 4) && rd(f, sigma2.data(), n_levels));
  fclose(f);
  fisheye.type = 1;   // GeometricCamera::CAM_FISHEYE
  memcpy(fisheye.K, pinhole.K, sizeof(pinhole.K));

  // key frame 1 observes point i at feature i; key frame 2 observes its match at feature n1 - 1 - i
  std::vector<MapPoint> p1(n1), p2(n1);
  std::vector<MapPoint*> matched(n1, nullptr);
  kf1.mpCamera = kf2.mpCamera = &pinhole;
  kf1.mvLevelSigma2 = kf2.mvLevelSigma2 = sigma2;
  kf1.mvpMapPoints.assign(n1, nullptr);
  kf1.mvKeysUn.resize(n1); kf2.mvKeysUn.resize(n1);
  int N = 0;
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
    if (state[i] == 4) ++N;
  }

  // 1. the second overload in steps of 20: what goes to the Python side
  test_rng::seed((unsigned)seed);
  Solver s1(&kf1, &kf2, matched, fix_scale != 0);
  s1.SetRansacParameters(0.99, min_inliers, 300);
  CHECK(s1.GetN() == N);
  const int max_its = s1.GetMaxIterations();
  const std::vector<CallRecord> calls = run_all(s1, 20);
  const int raw_draws = (int)test_rng::draws;   // rand() values used: after an early convergence more than the reference's
  CHECK(!calls.empty() && (calls.back().no_more || calls.back().converge));
  const M4 best1 = s1.GetEstimatedTransformation();
  if (calls.back().converge) {
    CHECK(same(best1, calls.back().T) && (!fix_scale || s1.GetEstimatedScale() == 1.0f));
    const M3 R = s1.GetEstimatedRotation();
    const V3 t = s1.GetEstimatedTranslation();
    const float s = s1.GetEstimatedScale();
    for (int i = 0; i < 3; ++i) {
      CHECK(t(i) == best1(i, 3));
      for (int j = 0; j < 3; ++j) CHECK(s * R(i, j) == best1(i, j));
    }
  }

  // 2. the first overload and find: the same triples (same seed), the identity unless converged
  {
    test_rng::seed((unsigned)seed);
    Solver s2(&kf1, &kf2, matched, fix_scale != 0);
    s2.SetRansacParameters(0.99, min_inliers, 300);
    for (size_t k = 0; k < calls.size(); ++k) {
      bool nm = false; std::vector<bool> fl; int ni = -1;
      const M4 T = s2.iterate(20, nm, fl, ni);
      CHECK(nm == calls[k].no_more && ni == calls[k].inliers && fl == calls[k].flags);
      CHECK(calls[k].converge ? same(T, calls[k].T) : identity(T));
    }
    test_rng::seed((unsigned)seed);
    Solver s3(&kf1, &kf2, matched, fix_scale != 0);
    s3.SetRansacParameters(0.99, min_inliers, 300);
    std::vector<bool> fl; int ni = -1;
    const M4 T = s3.find(fl, ni);   // one call of up to mRansacMaxIts iterations: the same scan, not cut into steps
    CHECK(ni == calls.back().inliers && fl == calls.back().flags && s3.GetIterations() == calls.back().iterations);
    CHECK(calls.back().converge ? same(T, calls.back().T) : identity(T));
  }

  // 3. SolveBatch over three solvers (the other scale mode, another threshold) against single solvers with the same seed
  {
    const int mins[3] = {min_inliers, N, min_inliers / 2 + 1};
    const bool fix[3] = {fix_scale != 0, fix_scale == 0, fix_scale != 0};
    std::vector<CallRecord> single(3);
    test_rng::seed((unsigned)seed + 1u);
    for (int b = 0; b < 3; ++b) {
      Solver s(&kf1, &kf2, matched, fix[b]);
      s.SetRansacParameters(0.99, mins[b], 300);
      CallRecord& r = single[b];
      r.T = s.iterate(20, r.no_more, r.flags, r.inliers, r.converge);
    }
    test_rng::seed((unsigned)seed + 1u);
    Solver a(&kf1, &kf2, matched, fix[0]), b(&kf1, &kf2, matched, fix[1]), c(&kf1, &kf2, matched, fix[2]);
    a.SetRansacParameters(0.99, mins[0], 300); b.SetRansacParameters(0.99, mins[1], 300); c.SetRansacParameters(0.99, mins[2], 300);
    std::vector<Solver*> all = {&a, &b, &c};
    std::vector<M4> vT; std::vector<bool> vNoMore, vConv; std::vector<std::vector<bool> > vFlags; std::vector<int> vInl;
    CHECK(Solver::SolveBatch(all, 20, vT, vNoMore, vFlags, vInl, vConv));
    for (int k = 0; k < 3; ++k)
      CHECK(same(vT[k], single[k].T) && vNoMore[k] == single[k].no_more && vConv[k] == single[k].converge && vInl[k] == single[k].inliers && vFlags[k] == single[k].flags);
  }

  // 4. a DeviceLocalMap, half of the points registered beforehand, against host arrays
  {
    rgbl_shim::DeviceLocalMap map(0, 64);
    std::vector<MapPoint*> some;
    for (int i = 0; i < n1; i += 2) { some.push_back(&p1[i]); some.push_back(&p2[i]); }
    CHECK(map.Update(some));
    test_rng::seed((unsigned)seed);
    Solver s(&kf1, &kf2, matched, fix_scale != 0, std::vector<KeyFrame*>(), &map);
    s.SetRansacParameters(0.99, min_inliers, 300);
    const std::vector<CallRecord> again = run_all(s, 20);
    CHECK(again.size() == calls.size() && (N < min_inliers || map.size() > some.size()));   // the other half was uploaded on the spot
    for (size_t k = 0; k < calls.size(); ++k)
      CHECK(same(again[k].T, calls[k].T) && again[k].flags == calls[k].flags && again[k].inliers == calls[k].inliers && again[k].samples == calls[k].samples);
  }

  // 5. N < mRansacMinInliers: over at once, nothing drawn; vpKeyFrameMatchedMP given: the same correspondences
  {
    test_rng::seed((unsigned)seed);
    const int first = test_rng::next();
    test_rng::seed((unsigned)seed);
    Solver s(&kf1, &kf2, matched, true, std::vector<KeyFrame*>(n1, &kf2));
    CHECK(s.GetN() == N);
    s.SetRansacParameters(0.99, N + 1, 300);
    bool nm = false, cv = true; std::vector<bool> fl; int ni = -1;
    const M4 T = s.iterate(20, nm, fl, ni, cv);
    CHECK(nm && !cv && ni == 0 && identity(T) && (int)fl.size() == n1 && s.GetIterations() == 0);
    CHECK(test_rng::next() == first);
  }

  // 6. a call after the iterations are used up runs nothing and returns mBestT12
  {
    test_rng::seed((unsigned)seed);
    Solver s(&kf1, &kf2, matched, fix_scale != 0);
    s.SetRansacParameters(0.99, N, 7);   // c > N never holds: runs through; mRansacMinInliers == N makes it one iteration
    CHECK(s.GetMaxIterations() == 1);
    bool nm = false, cv = true; std::vector<bool> fl; int ni = -1;
    const M4 T1 = s.iterate(20, nm, fl, ni, cv);
    CHECK(nm && !cv && s.GetIterations() == 1 && same(T1, s.GetEstimatedTransformation()));
    const M4 T2 = s.iterate(20, nm, fl, ni, cv);
    CHECK(nm && !cv && s.GetIterations() == 1 && same(T2, T1) && s.GetLastSamples().empty());
  }

  // 7. refused: a camera that is not a Pinhole
  {
    KeyFrame kf3 = kf2;
    kf3.mpCamera = &fisheye;
    for (int i = 0; i < n1; ++i) p2[i].kf = &kf3;
    Solver s(&kf1, &kf3, matched, true);
    bool nm = false, cv = true; std::vector<bool> fl; int ni = -1;
    const M4 T = s.iterate(20, nm, fl, ni, cv);
    CHECK(nm && !cv && ni == 0 && identity(T));
    std::vector<Solver*> all = {&s};
    std::vector<M4> vT; std::vector<bool> vNoMore, vConv; std::vector<std::vector<bool> > vFlags; std::vector<int> vInl;
    CHECK(!Solver::SolveBatch(all, 20, vT, vNoMore, vFlags, vInl, vConv) && vNoMore[0] && identity(vT[0]));
    for (int i = 0; i < n1; ++i) p2[i].kf = &kf2;
  }

  FILE* o = fopen(argv[2], "wb");
  CHECK(o);
  const int head[4] = {max_its, N, (int)calls.size(), raw_draws};
  fwrite(head, sizeof(int), 4, o);
  for (const CallRecord& r : calls) {
    const int rec[6] = {(int)r.samples.size() / 3, r.no_more ? 1 : 0, r.converge ? 1 : 0, r.inliers, r.iterations, r.best};
    fwrite(rec, sizeof(int), 6, o);
    fwrite(r.samples.data(), sizeof(int32_t), r.samples.size(), o);
    fwrite(r.T.m, sizeof(float), 16, o);
    std::vector<uint8_t> fl(n1);
    for (int i = 0; i < n1; ++i) fl[i] = r.flags[i] ? 1 : 0;
    fwrite(fl.data(), 1, n1, o);
  }
  fclose(o);
  rgbl_matcher_pool_clear();
  printf("SIM3_SHIM_OK %d calls, %d iterations of at most %d, %d inliers of %d\n", (int)calls.size(), calls.back().iterations, max_its, calls.back().inliers, N);
  return 0;
}
