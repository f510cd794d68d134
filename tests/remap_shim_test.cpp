// rgbl_shim::StereoRectifier and ORB_SLAM3::ORBextractor::ExtractRectified (orb_slam3_rgbl_amd/shim) used the way
// System::TrackStereo would use them, against the scalar restatement of cv::remap (tests/remap_ref.cpp, compiled in).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ORBextractor.h"
#include "StereoRectifier.h"

extern "C" int remap_ref(const uint8_t* src, int sw, int sh, int sstride, int cn, const float* mx, const float* my, int mstride,
                         uint8_t* dst, int dw, int dh, int dstride);

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  const int sw = 340, sh = 262, dw = 320, dh = 240;
  // a textured raw frame: blocks of random brightness with a gradient, so that FAST finds corners
  cv::Mat raw(sh, sw, CV_8UC1);
  unsigned rng = 7;
  std::vector<int> block((sw / 12 + 1) * (sh / 12 + 1));
  for (int& b : block) { rng = rng * 1664525u + 1013904223u; b = (rng >> 24) & 0xff; }
  for (int y = 0; y < sh; ++y)
    for (int x = 0; x < sw; ++x) raw.at<uint8_t>(y, x) = (uint8_t)((block[(y / 12) * (sw / 12 + 1) + x / 12] * 3 + x + y) / 4);
  // rotation by 3 degrees + radial distortion about the image centres
  cv::Mat M1(dh, dw, CV_32FC1), M2(dh, dw, CV_32FC1);
  const double f = 45.0 * dw / 83, a = 3.0 * M_PI / 180;
  for (int y = 0; y < dh; ++y)
    for (int x = 0; x < dw; ++x) {
      const double xn = (x - (dw - 1) / 2.0) / f, yn = (y - (dh - 1) / 2.0) / f;
      const double xr = cos(a) * xn - sin(a) * yn, yr = sin(a) * xn + cos(a) * yn, r2 = xr * xr + yr * yr, d = 1 + 0.35 * r2 + 0.05 * r2 * r2;
      M1.at<float>(y, x) = (float)(f * xr * d + (sw - 1) / 2.0);
      M2.at<float>(y, x) = (float)(f * yr * d + (sh - 1) / 2.0);
    }
  M1.at<float>(5, 7) = NAN; M2.at<float>(9, 300) = -INFINITY; M1.at<float>(200, 100) = 3e38f;

  rgbl_shim::StereoRectifier rect(M1, M2, cv::Size(sw, sh));
  CHECK(rect.ok());
  cv::Mat want(dh, dw, CV_8UC1), got;
  CHECK(remap_ref(raw.data, sw, sh, (int)raw.step, 1, M1.ptr<float>(0), M2.ptr<float>(0), dw, want.data, dw, dh, (int)want.step) == 0);
  CHECK(rect.remap(raw, got));
  CHECK(got.rows == dh && got.cols == dw && memcmp(got.data, want.data, (size_t)dw * dh) == 0);
  CHECK(got.at<uint8_t>(5, 7) == 0 && got.at<uint8_t>(9, 300) == 0 && got.at<uint8_t>(200, 100) == 0);
  cv::Mat small(10, 10, CV_8UC1), none;
  CHECK(!rect.remap(small, none));   // an image the maps were not built for

  ORB_SLAM3::ORBextractor raw_ex(500, 1.2f, 4, 20, 7), ref_ex(500, 1.2f, 4, 20, 7);
  std::vector<int> lap = {0, 0};
  std::vector<cv::KeyPoint> k1, k2;
  cv::Mat d1, d2, gray;
  for (int round = 0; round < 2; ++round) {
    const int m1 = raw_ex.ExtractRectified(rect, raw.data, 1, (int)raw.step, true, gray, k1, d1, lap);
    const int m2 = ref_ex(want, cv::Mat(), k2, d2, lap);
    CHECK(m1 == m2 && k1.size() == k2.size() && k1.size() > 50);
    CHECK(memcmp(gray.data, want.data, (size_t)dw * dh) == 0);
    CHECK(memcmp(k1.data(), k2.data(), k1.size() * sizeof(cv::KeyPoint)) == 0);
    CHECK(memcmp(d1.data, d2.data, k1.size() * 32) == 0);
  }
  printf("REMAP_SHIM_OK %zu keypoints\n", k1.size());
  return 0;
}
