// The reference's own TwoViewReconstruction functions (tests/_build/twoview_ref_bodies.inc, cut by tests/twoview_golden.py, never
// committed) compiled unmodified against tests/twoview_ref_types.h, as a program:   twoview_ref <case.bin> <out.bin>
// case.bin: int32 n1, n2, calls, iterations; float K[4], sigma; per call xy1 (n1 x 2 floats), xy2 (n2 x 2), matches12 (n1 int32).
// One object runs the calls one after the other, as Pinhole::ReconstructWithTwoViews keeps its tvr: DUtils::Random's stream goes on.
// out.bin per call: int32 ret, T21 assigned, vP3D.size(), vbTriangulated.size(); T21 (R row-major, t: 12 floats); mvSets
// (iterations x 8 int32); vbTriangulated (n1 bytes, 7 where the vector is shorter); vP3D; then what Reconstruct keeps to itself,
// from a second run of FindHomography and FindFundamental on the object's state: SH, SF, H (9), F (9), the H mask's size and N bytes,
// the F mask's size and N bytes (size 0: FindFundamental's quirk); and, where SF > 0, nGood[4] and parallax[4] of :484-503.
// At the end: how often acos(float) and acos(double) were bound.
#include <stdint.h>
#include <stdio.h>

#include "twoview_ref_types.h"

using namespace std;
namespace ORB_SLAM3 { int g_acos_float = 0, g_acos_double = 0; }
#include "twoview_ref_bodies.inc"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int32_t n1, n2, calls, iterations;
  float K[4], sigma;
  if (!rd(f, &n1, 1) || !rd(f, &n2, 1) || !rd(f, &calls, 1) || !rd(f, &iterations, 1) || !rd(f, K, 4) || !rd(f, &sigma, 1)) return 3;
  Eigen::Matrix3f Km;
  Km(0, 0) = K[0]; Km(1, 1) = K[1]; Km(0, 2) = K[2]; Km(1, 2) = K[3]; Km(2, 2) = 1.f;
  ORB_SLAM3::TwoViewReconstruction tvr(Km, sigma, iterations);
  for (int c = 0; c < calls; ++c) {
    std::vector<float> xy1(2 * (size_t)n1), xy2(2 * (size_t)n2);
    std::vector<int32_t> m((size_t)n1);
    if (!rd(f, xy1.data(), xy1.size()) || !rd(f, xy2.data(), xy2.size()) || !rd(f, m.data(), m.size())) return 3;
    std::vector<cv::KeyPoint> k1((size_t)n1), k2((size_t)n2);
    for (int i = 0; i < n1; ++i) { k1[(size_t)i].pt.x = xy1[2 * (size_t)i]; k1[(size_t)i].pt.y = xy1[2 * (size_t)i + 1]; }
    for (int i = 0; i < n2; ++i) { k2[(size_t)i].pt.x = xy2[2 * (size_t)i]; k2[(size_t)i].pt.y = xy2[2 * (size_t)i + 1]; }
    std::vector<int> matches(m.begin(), m.end());
    Sophus::SE3f T21;
    std::vector<cv::Point3f> vP3D;
    std::vector<bool> tri;
    const bool ret = tvr.Reconstruct(k1, k2, matches, T21, vP3D, tri);
    const int32_t head[4] = {ret ? 1 : 0, T21.assigned ? 1 : 0, (int32_t)vP3D.size(), (int32_t)tri.size()};
    wr(o, head, 4);
    wr(o, T21.R.m, 9); wr(o, T21.t.v, 3);
    for (const std::vector<size_t>& s : tvr.mvSets) for (size_t v : s) { const int32_t x = (int32_t)v; wr(o, &x, 1); }
    std::vector<uint8_t> flags((size_t)n1, 7);
    for (size_t i = 0; i < tri.size(); ++i) flags[i] = tri[i] ? 1 : 0;
    wr(o, flags.data(), flags.size());
    for (const cv::Point3f& p : vP3D) { const float x[3] = {p.x, p.y, p.z}; wr(o, x, 3); }
    // what Reconstruct keeps to itself
    std::vector<bool> vbH, vbF;
    float SH = 0, SF = 0;
    Eigen::Matrix3f H, F;
    tvr.FindHomography(vbH, SH, H);
    tvr.FindFundamental(vbF, SF, F);
    wr(o, &SH, 1); wr(o, &SF, 1); wr(o, H.m, 9); wr(o, F.m, 9);
    const int32_t N = (int32_t)tvr.mvMatches12.size();
    for (const std::vector<bool>* v : {&vbH, &vbF}) {
      const int32_t size = (int32_t)v->size();
      std::vector<uint8_t> b((size_t)N, 0);
      for (size_t i = 0; i < v->size() && i < (size_t)N; ++i) b[i] = (*v)[i] ? 1 : 0;
      wr(o, &size, 1);
      wr(o, b.data(), b.size());
    }
    int32_t nGood[4] = {0, 0, 0, 0};
    float par[4] = {0, 0, 0, 0};
    if (SF > 0) {   // :484-503
      Eigen::Matrix3f E21 = tvr.mK.transpose() * F * tvr.mK, R1, R2;
      Eigen::Vector3f t;
      tvr.DecomposeE(E21, R1, R2, t);
      Eigen::Vector3f t1 = t, t2 = -t;
      const Eigen::Matrix3f* Rs[4] = {&R1, &R2, &R1, &R2};
      const Eigen::Vector3f* ts[4] = {&t1, &t1, &t2, &t2};
      for (int j = 0; j < 4; ++j) {
        std::vector<cv::Point3f> P;
        std::vector<bool> g;
        nGood[j] = tvr.CheckRT(*Rs[j], *ts[j], tvr.mvKeys1, tvr.mvKeys2, tvr.mvMatches12, vbF, tvr.mK, P, 4.0 * tvr.mSigma2, g, par[j]);
      }
    }
    wr(o, nGood, 4); wr(o, par, 4);
  }
  const int32_t tail[2] = {ORB_SLAM3::g_acos_float, ORB_SLAM3::g_acos_double};
  wr(o, tail, 2);
  fclose(f);
  fclose(o);
  printf("TWOVIEW_REF_OK\n");
  return 0;
}
