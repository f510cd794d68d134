// resize_tab.h — cv::resize's fixed-point coefficient table of one axis (modules/imgproc/src/resize.cpp, INTER_LINEAR,
// 8-bit), shared by the pyramid (extractor.hip: k_resize_linear) and the ingest resize (resize.hip: k_resize_image).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace rgbl {

struct ResizeTab {  // one output column / row of cv::resize's fixed-point tables
  int32_t sofs;     // first source index
  int16_t a0, a1;   // 11-bit weights (sum 2048)
};

// Appends the dsize entries of one axis.  clamp_x: the x axis pulls its index into the row (and drops the fraction there);
// the y axis keeps sofs = -1 .. ssize - 1 and the reader clamps the two rows sofs, sofs + 1.
inline void build_resize_tab(int ssize, int dsize, bool clamp_x, std::vector<ResizeTab>& tab) {
  const double inv_scale = (double)dsize / ssize;
  const double scale = 1.0 / inv_scale;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)f;
    s -= f < (float)s;   // cvFloor
    f -= s;
    if (clamp_x) {
      if (s < 0) { f = 0; s = 0; }
      if (s >= ssize - 1) { f = 0; s = ssize - 1; }
    }
    ResizeTab t;
    t.sofs = s;
    t.a0 = (int16_t)lrintf((1.f - f) * 2048);   // cvRound: half to even
    t.a1 = (int16_t)lrintf(f * 2048);
    tab.push_back(t);
  }
}

}  // namespace rgbl
