// The drop-in rgbl_shim::TwoViewReconstruction (shim/TwoViewReconstruction.h) on stand-in types, as a program:
//   twoview_shim <case.bin> <out.bin> <assign_p3d_on_homography>
// case.bin as tests/twoview_ref_glue.cpp reads it: int32 n1, n2, calls, iterations; float K[4], sigma; then per call xy1 (n1 x 2 floats), xy2
// (n2 x 2), matches12 (n1 int32).
// One solver object runs the calls one after the other (the random stream goes on from call to call).  out.bin, per call: int32
// ret, model, exit_code, best_h, best_f, n_inliers, best_motion, p3d_size; float SH, SF; T21 (12 floats: R row-major, t);
// n_good[8]; parallax[8]; the sets (iterations x 8 int32); vbTriangulated (n1 bytes, 7 = the caller's vector was not touched);
// vP3D (p3d_size x 3 floats).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "TwoViewReconstruction.h"

namespace cv {
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; };
struct Point3f { float x = 0, y = 0, z = 0; Point3f() {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
}  // namespace cv
namespace Eigen {
struct Matrix3f { float m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; float& operator()(int r, int c) { return m[3 * r + c]; } float operator()(int r, int c) const { return m[3 * r + c]; } };
struct Vector3f { float v[3] = {0, 0, 0}; float& operator()(int i) { return v[i]; } float operator()(int i) const { return v[i]; } };
}  // namespace Eigen
namespace Sophus {
struct SE3f { Eigen::Matrix3f R; Eigen::Vector3f t; bool set = false; SE3f() {} SE3f(const Eigen::Matrix3f& r, const Eigen::Vector3f& tt) : R(r), t(tt), set(true) {} };
}  // namespace Sophus
typedef rgbl_shim::TwoViewReconstruction<Eigen::Matrix3f, Eigen::Vector3f, Sophus::SE3f, cv::KeyPoint, cv::Point3f> TwoViewReconstruction;

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  int32_t n1, n2, calls, iterations;
  float K[4], sigma;
  if (!rd(f, &n1, 1) || !rd(f, &n2, 1) || !rd(f, &calls, 1) || !rd(f, &iterations, 1) || !rd(f, K, 4) || !rd(f, &sigma, 1)) return 3;
  Eigen::Matrix3f Km;
  Km(0, 0) = K[0]; Km(1, 1) = K[1]; Km(0, 2) = K[2]; Km(1, 2) = K[3]; Km(2, 2) = 1.f;
  TwoViewReconstruction tvr(Km, sigma, iterations, argv[3][0] == '1');
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
    const rgbl_two_view_output& L = tvr.Last();
    if (ret != (L.found != 0) || ret != T21.set) return 4;
    const int32_t head[8] = {ret ? 1 : 0, L.model, L.exit_code, L.best_h, L.best_f, L.n_inliers, L.best_motion, (int32_t)vP3D.size()};
    wr(o, head, 8);
    wr(o, &L.SH, 1); wr(o, &L.SF, 1);
    wr(o, T21.R.m, 9); wr(o, T21.t.v, 3);
    wr(o, L.n_good, 8); wr(o, L.parallax, 8);
    wr(o, tvr.Sets().data(), tvr.Sets().size());
    std::vector<uint8_t> flags((size_t)n1, 7);
    for (size_t i = 0; i < tri.size(); ++i) flags[i] = tri[i] ? 1 : 0;
    wr(o, flags.data(), flags.size());
    for (const cv::Point3f& p : vP3D) { const float x[3] = {p.x, p.y, p.z}; wr(o, x, 3); }
  }
  fclose(f);
  fclose(o);
  printf("TWOVIEW_SHIM_OK\n");
  return 0;
}
