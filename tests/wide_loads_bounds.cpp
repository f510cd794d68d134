// Window bounds of k_gauss7 and k_resize_linear under AddressSanitizer (tests/test_wide_loads.py builds this file together with
// the kernel sources and the SIMT emulator, -fsanitize=address, into one program and runs it).  The emulator's "device" memory is
// the heap, so rgbl_extract_batch_device reads the frames where this program put them: blocks of exactly batch * width * height
// bytes, pitch == width, no byte behind the last row of the last frame.  A source window that leaves the image is a
// heap-buffer-overflow report and a non-zero exit status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rgbl_frontend.h"

struct Case { int w, h, levels; float scale; int batch; };

static int run(const Case& c) {
  rgbl_extractor_cfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.nfeatures = 100; cfg.scale_factor = c.scale; cfg.nlevels = c.levels; cfg.ini_th_fast = 20; cfg.min_th_fast = 7;
  cfg.width = c.w; cfg.height = c.h; cfg.max_batch = c.batch;
  rgbl_extractor* ex = nullptr;
  if (rgbl_extractor_create(&cfg, 0, &ex) != RGBL_OK) { printf("create %dx%d: %s\n", c.w, c.h, rgbl_last_error()); return 1; }
  const size_t frame = (size_t)c.w * c.h;
  uint8_t* imgs = (uint8_t*)malloc(frame * c.batch);   // exactly the frames
  uint32_t s = 12345u + (uint32_t)c.w;
  for (size_t i = 0; i < frame * c.batch; ++i) { s = s * 1664525u + 1013904223u; imgs[i] = (uint8_t)(s >> 24); }
  const int cap = rgbl_extractor_max_keypoints(ex);
  rgbl_keypoint* kp = (rgbl_keypoint*)malloc(sizeof(rgbl_keypoint) * (size_t)cap * c.batch);
  uint8_t* desc = (uint8_t*)malloc((size_t)cap * 32 * c.batch);
  int32_t* n = (int32_t*)malloc(sizeof(int32_t) * c.batch);
  int32_t* mono = (int32_t*)malloc(sizeof(int32_t) * c.batch);
  int rc = rgbl_extract_batch_device(ex, imgs, c.batch, c.w, c.h, c.w, frame, 0, 0, kp, desc, cap, n, mono);
  if (rc == RGBL_OK) rc = rgbl_extractor_sync(ex);
  if (rc != RGBL_OK) printf("extract %dx%d: %s\n", c.w, c.h, rgbl_last_error());
  long total = 0;
  for (int b = 0; rc == RGBL_OK && b < c.batch; ++b) total += n[b];
  printf("%4d x %3d, %d levels at %.1f, %d frames: %ld keypoints\n", c.w, c.h, c.levels, c.scale, c.batch, total);
  if (rc == RGBL_OK && total == 0) { printf("no keypoints: the blur stage had nothing to do\n"); rc = 1; }
  free(mono); free(n); free(desc); free(kp); free(imgs);
  rgbl_extractor_destroy(ex);
  return rc != RGBL_OK;
}

int main() {
  // widths on both sides of a tile column and a multiple of 64 (the handle's own pitch), level 1 at every kind of pair
  // (window, pulled-back window, groups on their own), the smallest level, KITTI's eight levels
  const Case cases[] = {{121, 99, 2, 1.2f, 3}, {128, 97, 2, 1.1f, 2}, {141, 101, 2, 1.5f, 2}, {139, 134, 2, 2.0f, 2},
                        {80, 81, 2, 1.2f, 3}, {1241, 376, 8, 1.2f, 2}};
  for (const Case& c : cases)
    if (run(c)) return 1;
  printf("bounds ok\n");
  return 0;
}
