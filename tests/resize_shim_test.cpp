// rgbl_shim::ImageResizer and ORB_SLAM3::ORBextractor::ExtractResized (orb_slam3_rgbl_amd/shim) used the way the System::Track*
// entries would use them, against a scalar restatement of cv::resize written out here (INTER_LINEAR, one channel; the same
// arithmetic as tests/resize_ref.py and the oracle, a restatement, unpinned).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ImageResizer.h"
#include "ORBextractor.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void axis(int ssize, int dsize, bool clamp, std::vector<int>& s, std::vector<int>& a0, std::vector<int>& a1) {
  const double scale = 1.0 / ((double)dsize / ssize);
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int i = (int)floorf(f);
    f -= i;
    if (clamp && i < 0) { i = 0; f = 0; }
    if (clamp && i >= ssize - 1) { i = ssize - 1; f = 0; }
    s.push_back(i); a0.push_back((int)lrintf((1.f - f) * 2048)); a1.push_back((int)lrintf(f * 2048));
  }
}

static cv::Mat resize_ref(const cv::Mat& src, int dw, int dh) {
  std::vector<int> sx, xa0, xa1, sy, ya0, ya1;
  axis(src.cols, dw, true, sx, xa0, xa1);
  axis(src.rows, dh, false, sy, ya0, ya1);
  cv::Mat dst(dh, dw, CV_8UC1);
  auto h = [&](int y, int dx) {
    y = y < 0 ? 0 : y > src.rows - 1 ? src.rows - 1 : y;
    const int x1 = sx[dx] + 1 < src.cols ? sx[dx] + 1 : src.cols - 1;
    return src.at<uint8_t>(y, sx[dx]) * xa0[dx] + src.at<uint8_t>(y, x1) * xa1[dx];
  };
  for (int dy = 0; dy < dh; ++dy)
    for (int dx = 0; dx < dw; ++dx)
      dst.at<uint8_t>(dy, dx) = (uint8_t)((((ya0[dy] * (h(sy[dy], dx) >> 4)) >> 16) + ((ya1[dy] * (h(sy[dy] + 1, dx) >> 4)) >> 16) + 2) >> 2);
  return dst;
}

int main() {
  const int sw = 400, sh = 300, dw = 320, dh = 240;
  // a textured raw frame: blocks of random brightness with a gradient, so that FAST finds corners
  cv::Mat raw(sh, sw, CV_8UC1);
  unsigned rng = 7;
  std::vector<int> block((sw / 12 + 1) * (sh / 12 + 1));
  for (int& b : block) { rng = rng * 1664525u + 1013904223u; b = (rng >> 24) & 0xff; }
  for (int y = 0; y < sh; ++y)
    for (int x = 0; x < sw; ++x) raw.at<uint8_t>(y, x) = (uint8_t)((block[(y / 12) * (sw / 12 + 1) + x / 12] * 3 + x + y) / 4);

  rgbl_shim::ImageResizer resizer(cv::Size(sw, sh), cv::Size(dw, dh));
  CHECK(resizer.ok() && resizer.srcWidth() == sw && resizer.srcHeight() == sh && resizer.dstWidth() == dw && resizer.dstHeight() == dh);
  const cv::Mat want = resize_ref(raw, dw, dh);
  cv::Mat got;
  CHECK(resizer.resize(raw, got));
  CHECK(got.rows == dh && got.cols == dw && memcmp(got.data, want.data, (size_t)dw * dh) == 0);
  cv::Mat small(10, 10, CV_8UC1), none;
  CHECK(!resizer.resize(small, none));   // an image of another size
  rgbl_shim::ImageResizer bad(cv::Size(0, sh), cv::Size(dw, dh));
  CHECK(!bad.ok() && !bad.resize(raw, none));   // reports, never throws

  // Settings.cc:364-404 at the reference's EuRoC sizes (Examples/Monocular/EuRoC.yaml: 752 x 480 -> 600 x 350, Camera1.*)
  rgbl_shim::ImageResizer euroc(cv::Size(752, 480), cv::Size(600, 350));
  float fx = 458.654f, fy = 457.296f, cx = 367.215f, cy = 248.375f;
  euroc.ScaleCalibration(fx, fy, cx, cy);
  CHECK(fx == 458.654f * ((float)600 / (float)752) && cx == 367.215f * ((float)600 / (float)752));
  CHECK(fy == 457.296f * ((float)350 / (float)480) && cy == 248.375f * ((float)350 / (float)480));
  float l0 = 0.f, l1 = 511.f;
  euroc.ScaleLappingArea(l0, l1);
  CHECK(l0 == 0.f && l1 == 511.f * ((float)600 / (float)752));

  ORB_SLAM3::ORBextractor raw_ex(500, 1.2f, 4, 20, 7), ref_ex(500, 1.2f, 4, 20, 7);
  std::vector<int> lap = {0, 0};
  std::vector<cv::KeyPoint> k1, k2;
  cv::Mat d1, d2, gray;
  for (int round = 0; round < 2; ++round) {
    const int m1 = raw_ex.ExtractResized(resizer, raw.data, 1, (int)raw.step, true, gray, k1, d1, lap);
    const int m2 = ref_ex(want, cv::Mat(), k2, d2, lap);
    CHECK(m1 == m2 && k1.size() == k2.size() && k1.size() > 50);
    CHECK(memcmp(gray.data, want.data, (size_t)dw * dh) == 0);
    CHECK(memcmp(k1.data(), k2.data(), k1.size() * sizeof(cv::KeyPoint)) == 0);
    CHECK(memcmp(d1.data, d2.data, k1.size() * 32) == 0);
  }
  CHECK(raw_ex.ExtractResized(bad, raw.data, 1, (int)raw.step, true, gray, k1, d1, lap) == -1);
  printf("RESIZE_SHIM_OK %zu keypoints\n", k2.size());
  return 0;
}
