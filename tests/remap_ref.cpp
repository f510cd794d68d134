// remap_ref.cpp — cv::remap(src, dst, map_x, map_y, cv::INTER_LINEAR, cv::BORDER_CONSTANT, 0) for CV_8UC{1,3,4} with two
// CV_32FC1 maps, restated as scalar C++ in the shape of OpenCV 4.x imgproc/src/remap.cpp: the 32 x 32 table of 15-bit
// `short` weights (initInterTab2D), the float -> fixed-point conversion of RemapInvoker, and the three branches of
// remapBilinear (all taps inside / all taps outside / every tap tested).  Written independently of tests/remap_ref.py;
// tests/test_remap_restatements.py compares the two.  A restatement, unpinned: no OpenCV is available to the build.
//
// One known simplification: initInterTab2D repairs entries whose rounded weights do not sum to 2^15.  With 32 steps per
// axis every product is an exact multiple of 32, so the only such entry is (0, 0), whose single weight 32768 saturates to
// 32767 in the `short`; it is kept at 32767 here ((v * 32767 + 2^14) >> 15 == v for every 8-bit v).
#include <stdint.h>
#include <xmmintrin.h>

namespace {

const int kTabSize = 32, kCoefBits = 15, kCoefScale = 1 << kCoefBits;
short g_tab[kTabSize * kTabSize][4];
bool g_tab_ready = false;

short saturate_short(int v) { return (short)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }
int cv_round(float v) { return _mm_cvtss_si32(_mm_set_ss(v)); }   // cvtss2si: what OpenCV's cvRound is on x86

void init_tab() {
  if (g_tab_ready) return;
  float lin[kTabSize][2];
  for (int i = 0; i < kTabSize; ++i) {   // interpolateLinear(i / 32)
    const float x = (float)i * (1.f / kTabSize);
    lin[i][0] = 1.f - x;
    lin[i][1] = x;
  }
  for (int i = 0; i < kTabSize; ++i)       // i: fraction of y
    for (int j = 0; j < kTabSize; ++j)     // j: fraction of x
      for (int k1 = 0; k1 < 2; ++k1)
        for (int k2 = 0; k2 < 2; ++k2) {
          const float v = lin[i][k1] * lin[j][k2];
          g_tab[i * kTabSize + j][k1 * 2 + k2] = saturate_short(cv_round(v * kCoefScale));
        }
  g_tab_ready = true;
}

inline uint8_t fixed_cast(int v) {   // FixedPtCast<int, uchar, 15>
  v = (v + (1 << (kCoefBits - 1))) >> kCoefBits;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

}  // namespace

extern "C" int remap_ref(const uint8_t* src, int sw, int sh, int sstride, int cn, const float* mx, const float* my, int mstride,
                         uint8_t* dst, int dw, int dh, int dstride) {
  if (cn != 1 && cn != 3 && cn != 4) return -1;
  init_tab();
  const int width1 = sw - 1 > 0 ? sw - 1 : 0, height1 = sh - 1 > 0 ? sh - 1 : 0;
  for (int dy = 0; dy < dh; ++dy) {
    uint8_t* D = dst + (size_t)dy * dstride;
    for (int dx = 0; dx < dw; ++dx, D += cn) {
      // RemapInvoker, CV_32FC1 pair + INTER_LINEAR: XY = saturate_cast<short>(s >> 5), FXY = (sy & 31) * 32 + (sx & 31)
      const int fsx = cv_round(mx[(size_t)dy * mstride + dx] * kTabSize), fsy = cv_round(my[(size_t)dy * mstride + dx] * kTabSize);
      const int sx = saturate_short(fsx >> 5), sy = saturate_short(fsy >> 5);
      const short* w = g_tab[(fsy & (kTabSize - 1)) * kTabSize + (fsx & (kTabSize - 1))];
      if ((unsigned)sx < (unsigned)width1 && (unsigned)sy < (unsigned)height1) {
        const uint8_t* S = src + (size_t)sy * sstride + sx * cn;
        for (int k = 0; k < cn; ++k)
          D[k] = fixed_cast(S[k] * w[0] + S[k + cn] * w[1] + S[sstride + k] * w[2] + S[sstride + k + cn] * w[3]);
      } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        for (int k = 0; k < cn; ++k) D[k] = 0;   // borderValue
      } else {
        const int sx0 = sx, sx1 = sx + 1, sy0 = sy, sy1 = sy + 1;
        const bool x0 = sx0 >= 0 && sx0 < sw, x1 = sx1 >= 0 && sx1 < sw, y0 = sy0 >= 0 && sy0 < sh, y1 = sy1 >= 0 && sy1 < sh;
        for (int k = 0; k < cn; ++k) {
          const int v0 = x0 && y0 ? src[(size_t)sy0 * sstride + sx0 * cn + k] : 0;
          const int v1 = x1 && y0 ? src[(size_t)sy0 * sstride + sx1 * cn + k] : 0;
          const int v2 = x0 && y1 ? src[(size_t)sy1 * sstride + sx0 * cn + k] : 0;
          const int v3 = x1 && y1 ? src[(size_t)sy1 * sstride + sx1 * cn + k] : 0;
          D[k] = fixed_cast(v0 * w[0] + v1 * w[1] + v2 * w[2] + v3 * w[3]);
        }
      }
    }
  }
  return 0;
}
