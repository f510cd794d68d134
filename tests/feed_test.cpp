// The host-fed batch front end driven from C++ through the C ABI alone (include/rgbl_frontend.h: rgbl_feeder_*), in the shape of
// the frame loop of Examples/RGB-L/rgbl_kitti.cc:87-125 (image + velodyne .bin scan read from files, one frame after another).
// Every frame is held to the single-frame ABI calls (rgbl_extract_color + rgbl_depth_compute_xyzi) on the same bytes.
//
//   feed_test <dir> <w> <h> <nfeatures> <nlevels> <frames> <batch> <slots> <max_points>
//   <dir>/proj.txt            LidarProjectionMatrix, 12 floats
//   <dir>/frame_NNNNNN.bgr    w x h x 3 bytes, BGR (what cv::imread hands GrabImageRGBL)
//   <dir>/scan_NNNNNN.bin     KITTI velodyne records (x, y, z, reflectance as float32)
// Prints FEED_CPP_OK <frames> <keypoints> <keypoints with depth> on success.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rgbl_frontend.h"

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    int rc__ = (x);                                                                                \
    if (rc__ != RGBL_OK) {                                                                         \
      fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #x, rc__, rgbl_last_error());   \
      exit(1);                                                                                     \
    }                                                                                              \
  } while (0)
#define EXPECT(c, ...)                    \
  do {                                    \
    if (!(c)) {                           \
      fprintf(stderr, __VA_ARGS__);       \
      fprintf(stderr, "\n");              \
      exit(2);                            \
    }                                     \
  } while (0)

static std::string path(const char* dir, const char* stem, int i, const char* ext) {
  char buf[64];
  snprintf(buf, sizeof buf, "/%s_%06d.%s", stem, i, ext);
  return std::string(dir) + buf;
}

int main(int argc, char** argv) {
  if (argc != 10) { fprintf(stderr, "usage: feed_test dir w h nfeatures nlevels frames batch slots max_points\n"); return 64; }
  const char* dir = argv[1];
  const int w = atoi(argv[2]), h = atoi(argv[3]), nfeatures = atoi(argv[4]), nlevels = atoi(argv[5]);
  const int n_frames = atoi(argv[6]), B = atoi(argv[7]), slots = atoi(argv[8]), max_points = atoi(argv[9]);

  float proj[12];
  FILE* pf = fopen((std::string(dir) + "/proj.txt").c_str(), "r");
  EXPECT(pf, "no proj.txt");
  for (float& v : proj) EXPECT(fscanf(pf, "%f", &v) == 1, "proj.txt: 12 floats");
  fclose(pf);

  // ORBextractor + DepthModule as Frame / Tracking construct them (KITTI00-02.yaml: InverseDilation, Diamond 5)
  auto make = [&](int batch, rgbl_extractor** ex, rgbl_depth** dm) {
    rgbl_extractor_cfg ec = {nfeatures, 1.2f, nlevels, 20, 7, w, h, batch};
    CHECK(rgbl_extractor_create(&ec, 0, ex));
    rgbl_depth_cfg dc;
    memset(&dc, 0, sizeof dc);
    memcpy(dc.proj, proj, sizeof proj);
    dc.min_dist = 5.0f; dc.max_dist = 200.0f; dc.mbf = 100.0f;
    dc.method = RGBL_UPS_INVERSE_DILATION;
    dc.kernel_w = dc.kernel_h = 5;
    CHECK(rgbl_structuring_element(3, 5, 5, dc.kernel));
    dc.avg_kernel_size = 5; dc.nn_search_radius = 7.0f;
    dc.width = w; dc.height = h; dc.max_points = max_points;
    dc.max_keypoints = rgbl_extractor_max_keypoints(*ex);
    dc.max_batch = batch;
    CHECK(rgbl_depth_create(&dc, 0, dm));
  };
  rgbl_extractor* ex; rgbl_depth* dm;
  make(B, &ex, &dm);
  rgbl_extractor* ex1; rgbl_depth* dm1;
  make(1, &ex1, &dm1);

  rgbl_feeder_cfg fc;
  memset(&fc, 0, sizeof fc);
  fc.channels = 3; fc.blue_first = 1;  // Camera.RGB: 0
  fc.max_batch = B; fc.max_points = max_points; fc.slots = slots;
  rgbl_feeder* fd;
  CHECK(rgbl_feeder_create(&fc, ex, dm, &fd));

  // the single-frame reference of one frame, from the same files
  const int cap1 = rgbl_extractor_max_keypoints(ex1);
  std::vector<uint8_t> img((size_t)w * h * 3), desc1((size_t)cap1 * 32);
  std::vector<rgbl_keypoint> kp1(cap1);
  std::vector<float> scan, xy, un, d1, u1;
  long long total_kp = 0, total_hits = 0;
  auto check_frame = [&](int frame, const rgbl_feeder_results& r, int b) {
    FILE* f = fopen(path(dir, "frame", frame, "bgr").c_str(), "rb");
    EXPECT(f && fread(img.data(), 1, img.size(), f) == img.size(), "frame %d", frame);
    fclose(f);
    f = fopen(path(dir, "scan", frame, "bin").c_str(), "rb");
    EXPECT(f, "scan %d", frame);
    fseek(f, 0, SEEK_END);
    const int n = (int)(ftell(f) / 16);
    rewind(f);
    scan.resize((size_t)4 * n + 4);
    EXPECT(fread(scan.data(), 16, n, f) == (size_t)n, "scan %d", frame);
    fclose(f);
    int k = 0, mono = 0;
    CHECK(rgbl_extract_color(ex1, img.data(), 3, 1, w, h, 3 * w, 0, 0, kp1.data(), desc1.data(), cap1, &k, &mono, nullptr, 0));
    xy.resize(2 * (size_t)k + 2); un.resize(k + 1); d1.resize(k + 1); u1.resize(k + 1);
    for (int i = 0; i < k; ++i) { xy[2 * i] = kp1[i].x; xy[2 * i + 1] = kp1[i].y; un[i] = kp1[i].x; }
    CHECK(rgbl_depth_compute_xyzi(dm1, scan.data(), n, w, h, xy.data(), un.data(), k, d1.data(), u1.data(), nullptr, nullptr));
    EXPECT(r.n[b] == k && r.mono[b] == mono, "frame %d: %d keypoints (mono %d), single-frame call %d (%d)", frame, r.n[b], r.mono[b], k, mono);
    EXPECT(!memcmp(r.kp + (size_t)b * r.cap, kp1.data(), sizeof(rgbl_keypoint) * k), "frame %d: keypoints differ", frame);
    EXPECT(!memcmp(r.desc + (size_t)b * r.cap * 32, desc1.data(), (size_t)k * 32), "frame %d: descriptors differ", frame);
    EXPECT(!memcmp(r.depth + (size_t)b * r.cap, d1.data(), sizeof(float) * k), "frame %d: mvDepth differs", frame);
    EXPECT(!memcmp(r.uright + (size_t)b * r.cap, u1.data(), sizeof(float) * k), "frame %d: mvuRight differs", frame);
    EXPECT(r.kpun_xy == nullptr, "no undistortion configured");
    total_kp += k;
    for (int i = 0; i < k; ++i) total_hits += d1[i] > 0;
  };

  // rgbl_kitti.cc's loop, B frames per step, `slots - 1` batches in flight behind the one being filled
  std::vector<int> first(slots, 0);
  std::vector<int> pending;  // slots in submit order
  auto collect = [&]() {
    const int s = pending.front();
    pending.erase(pending.begin());
    rgbl_feeder_results r;
    CHECK(rgbl_feeder_collect(fd, s, &r));
    for (int b = 0; b < r.batch; ++b) check_frame(first[s] + b, r, b);
  };
  for (int ni = 0; ni < n_frames; ni += B) {
    if ((int)pending.size() == slots) collect();
    int slot;
    CHECK(rgbl_feeder_acquire(fd, &slot));
    const int nb = std::min(B, n_frames - ni);
    for (int b = 0; b < nb; ++b) {
      FILE* f = fopen(path(dir, "scan", ni + b, "bin").c_str(), "rb");  // LoadPointcloudBinaryMat: size / 16 records
      EXPECT(f, "scan %d", ni + b);
      fseek(f, 0, SEEK_END);
      const int n = (int)(ftell(f) / 16);
      rewind(f);
      float* xyzi;
      CHECK(rgbl_feeder_scan(fd, slot, b, n, &xyzi));
      EXPECT(fread(xyzi, 16, n, f) == (size_t)n, "scan %d", ni + b);
      fclose(f);
      uint8_t* px;
      CHECK(rgbl_feeder_image(fd, slot, b, &px));
      f = fopen(path(dir, "frame", ni + b, "bgr").c_str(), "rb");  // a decoder would write here instead
      EXPECT(f && fread(px, 1, (size_t)w * h * 3, f) == (size_t)w * h * 3, "frame %d", ni + b);
      fclose(f);
    }
    CHECK(rgbl_feeder_submit(fd, slot, nb));
    first[slot] = ni;
    pending.push_back(slot);
  }
  while (!pending.empty()) collect();
  rgbl_feeder_destroy(fd);
  rgbl_extractor_destroy(ex); rgbl_depth_destroy(dm);
  rgbl_extractor_destroy(ex1); rgbl_depth_destroy(dm1);
  printf("FEED_CPP_OK %d %lld %lld\n", n_frames, total_kp, total_hits);
  return 0;
}
