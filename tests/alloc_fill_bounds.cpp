// RGBL_ALLOC_FILL under AddressSanitizer (tests/test_alloc_fill.py builds this file together with the kernel sources and the SIMT
// emulator, -fsanitize=address, into one program and runs it).  The switch is read once per process, so main() starts one child
// per byte (fork before the first library call), the child sets RGBL_ALLOC_FILL and makes one call each of the extractor, the
// depth module, the Hamming scan, SearchByProjection, the Sim3 RANSAC and the local bundle adjustment, with every input and
// output in a heap block of exactly its size.  The emulator's "device" memory is the heap: an index that a kernel reads from
// memory nobody wrote - 0xFFFFFFFF or 0x5A5A5A5A here, not a fresh page's zero - is a heap-buffer-overflow report and a non-zero
// exit status on the CPU, not a fault on a GPU.  Every child prints a checksum of each call's results; the two must agree.
#include <sys/wait.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "rgbl_frontend.h"

static uint32_t g_seed = 1;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static float unit() { return (float)(rnd() & 0xffff) / 65536.f; }
template <class T> static T* heap(size_t count) { return (T*)malloc(sizeof(T) * (count ? count : 1)); }   // exactly the array
static uint32_t sum_bytes(const void* p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 16777619u;
  return h;
}
#define CHECK(call)                                                           \
  do {                                                                        \
    if ((call) != RGBL_OK) { printf("%s: %s\n", #call, rgbl_last_error()); return 1; } \
  } while (0)

static int run_extractor() {
  const int w = 141, h = 101, batch = 2;
  rgbl_extractor_cfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.nfeatures = 100; cfg.scale_factor = 1.2f; cfg.nlevels = 2; cfg.ini_th_fast = 20; cfg.min_th_fast = 7;
  cfg.width = w; cfg.height = h; cfg.max_batch = batch;
  rgbl_extractor* ex = nullptr;
  CHECK(rgbl_extractor_create(&cfg, 0, &ex));
  const size_t frame = (size_t)w * h;
  uint8_t* imgs = heap<uint8_t>(frame * batch);
  for (size_t i = 0; i < frame * batch; ++i) imgs[i] = (uint8_t)rnd();
  const int cap = rgbl_extractor_max_keypoints(ex);
  rgbl_keypoint* kp = heap<rgbl_keypoint>((size_t)cap * batch);
  uint8_t* desc = heap<uint8_t>((size_t)cap * 32 * batch);
  int32_t *n = heap<int32_t>(batch), *mono = heap<int32_t>(batch);
  CHECK(rgbl_extract_batch_device(ex, imgs, batch, w, h, w, frame, 0, 0, kp, desc, cap, n, mono));
  CHECK(rgbl_extractor_sync(ex));
  uint32_t sum = 0;
  long total = 0;
  for (int b = 0; b < batch; ++b) {
    total += n[b];
    sum ^= sum_bytes(kp + (size_t)b * cap, sizeof(rgbl_keypoint) * n[b]) ^ sum_bytes(desc + (size_t)b * cap * 32, (size_t)32 * n[b]);
  }
  printf("extractor: %ld keypoints, checksum %08x\n", total, sum);
  free(mono); free(n); free(desc); free(kp); free(imgs);
  rgbl_extractor_destroy(ex);
  return total == 0;
}

static int run_depth() {
  const int w = 96, h = 64, n = 500, k = 40;
  rgbl_depth_cfg cfg;
  memset(&cfg, 0, sizeof(cfg));
  const float K[12] = {80, 0, w / 2.f, 0, 0, 80, h / 2.f, 0, 0, 0, 1, 0};
  const float Tr[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rgbl_projection_matrix(K, Tr, cfg.proj);
  cfg.min_dist = 5.f; cfg.max_dist = 200.f; cfg.mbf = 100.f; cfg.method = RGBL_UPS_INVERSE_DILATION;
  cfg.kernel_w = 5; cfg.kernel_h = 5;
  CHECK(rgbl_structuring_element(3, 5, 5, cfg.kernel));
  cfg.avg_kernel_size = 5; cfg.nn_search_radius = 7.f;
  cfg.width = w; cfg.height = h; cfg.max_points = n; cfg.max_keypoints = k; cfg.max_batch = 1;
  rgbl_depth* dm = nullptr;
  CHECK(rgbl_depth_create(&cfg, 0, &dm));
  float* cloud = heap<float>((size_t)4 * n);   // rows x, y, z, 1
  for (int i = 0; i < n; ++i) {
    const float z = 6.f + 60.f * unit();
    cloud[i] = (unit() - 0.5f) * z * 1.1f; cloud[n + i] = (unit() - 0.5f) * z * 0.7f; cloud[2 * n + i] = z; cloud[3 * n + i] = 1.f;
  }
  float *kp = heap<float>((size_t)2 * k), *kpx = heap<float>(k), *d = heap<float>(k), *ur = heap<float>(k);
  for (int i = 0; i < k; ++i) { kp[2 * i] = kpx[i] = 1.f + (w - 3) * unit(); kp[2 * i + 1] = 1.f + (h - 3) * unit(); }
  float *raw = heap<float>((size_t)w * h), *proc = heap<float>((size_t)w * h);
  CHECK(rgbl_depth_compute(dm, cloud, n, n, w, h, kp, kpx, k, d, ur, raw, proc));          // with the maps
  const uint32_t with_maps = sum_bytes(d, sizeof(float) * k) ^ sum_bytes(ur, sizeof(float) * k);
  CHECK(rgbl_depth_compute(dm, cloud, n, n, w, h, kp, kpx, k, d, ur, nullptr, nullptr));   // through the index map
  const uint32_t without = sum_bytes(d, sizeof(float) * k) ^ sum_bytes(ur, sizeof(float) * k);
  int hits = 0;
  for (int i = 0; i < k; ++i) hits += d[i] > 0;
  printf("depth: %d of %d keypoints with a depth, checksum %08x, maps %08x\n", hits, k, with_maps,
         sum_bytes(raw, sizeof(float) * w * h) ^ sum_bytes(proc, sizeof(float) * w * h));
  free(proc); free(raw); free(ur); free(d); free(kpx); free(kp); free(cloud);
  rgbl_depth_destroy(dm);
  return hits == 0 || with_maps != without;
}

static int popcount_row(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

static int run_hamming(rgbl_matcher* mt) {
  const int na = 130, nb = 513;   // nine 64-row stages: two launch slices, folded by k_hamming_merge
  uint8_t *a = heap<uint8_t>((size_t)na * 32), *b = heap<uint8_t>((size_t)nb * 32);
  for (int i = 0; i < na * 32; ++i) a[i] = (uint8_t)rnd();
  for (int i = 0; i < nb * 32; ++i) b[i] = (uint8_t)rnd();
  for (int j = 0; j < nb; j += 3) { memcpy(b + (size_t)j * 32, a + (size_t)((7 * j) % na) * 32, 32); b[(size_t)j * 32 + j % 32] ^= (uint8_t)(1u << (j % 8)); }
  int32_t *bi = heap<int32_t>(na), *bd = heap<int32_t>(na), *sd = heap<int32_t>(na);
  CHECK(rgbl_hamming_bf(mt, a, na, b, nb, bi, bd, sd));
  int bad = 0;
  for (int i = 0; i < na; ++i) {
    int best = 257, second = 257, idx = -1;
    for (int j = 0; j < nb; ++j) {
      const int d = popcount_row(a + (size_t)i * 32, b + (size_t)j * 32);
      if (d < best) { second = best; best = d; idx = j; } else if (d < second) second = d;
    }
    bad += bi[i] != idx || bd[i] != best || sd[i] != second;
  }
  printf("hamming: %d of %d rows differ from the plain scan, checksum %08x\n", bad, na, sum_bytes(bi, 4 * na) ^ sum_bytes(bd, 4 * na) ^ sum_bytes(sd, 4 * na));
  free(sd); free(bd); free(bi); free(b); free(a);
  return bad != 0;
}

// SearchByProjection(CurrentFrame, LastFrame): n1 map points in front of both cameras, the current frame's features on their
// projections (every third one somewhere else), the point's descriptor with a few bits flipped
static int run_projection(rgbl_matcher* mt) {
  const int n1 = 150, n2 = 170, levels = 8;
  rgbl_projection_input in;
  memset(&in, 0, sizeof(in));
  const float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f, W = 640.f, H = 480.f;
  uint8_t *valid = heap<uint8_t>(n1), *observed = heap<uint8_t>(n1), *mpd = heap<uint8_t>((size_t)n1 * 32), *desc2 = heap<uint8_t>((size_t)n2 * 32);
  float *wp = heap<float>((size_t)3 * n1), *ang1 = heap<float>(n1), *xy2 = heap<float>((size_t)2 * n2), *ang2 = heap<float>(n2), *ur2 = heap<float>(n2);
  int32_t *oct1 = heap<int32_t>(n1), *oct2 = heap<int32_t>(n2);
  float* sf = heap<float>(levels);
  for (int l = 0; l < levels; ++l) sf[l] = l ? sf[l - 1] * 1.2f : 1.f;
  const float tx = 0.05f;   // the current camera has moved 5 cm along x: Tcw translation -tx
  int planted = 0;
  for (int i = 0; i < n1; ++i) {
    const float z = 4.f + 20.f * unit(), x = (unit() - 0.5f) * z, y = (unit() - 0.5f) * z * 0.7f;
    wp[3 * i] = x; wp[3 * i + 1] = y; wp[3 * i + 2] = z;
    valid[i] = i % 11 != 0; observed[i] = i % 5 != 0; oct1[i] = i % 3; ang1[i] = 10.f * (i % 36);
    for (int k = 0; k < 32; ++k) mpd[(size_t)i * 32 + k] = (uint8_t)rnd();
  }
  for (int j = 0; j < n2; ++j) {
    for (int k = 0; k < 32; ++k) desc2[(size_t)j * 32 + k] = (uint8_t)rnd();
    xy2[2 * j] = W * unit(); xy2[2 * j + 1] = H * unit(); oct2[j] = j % 3; ang2[j] = 10.f * (j % 36); ur2[j] = -1.f;
    if (j < n1 && j % 3 != 2) {
      const float u = fx * (wp[3 * j] - tx) / wp[3 * j + 2] + cx, v = fy * wp[3 * j + 1] / wp[3 * j + 2] + cy;
      if (u < 1 || v < 1 || u > W - 2 || v > H - 2) continue;
      xy2[2 * j] = u + 0.4f; xy2[2 * j + 1] = v - 0.3f; ur2[j] = xy2[2 * j] - 40.f / wp[3 * j + 2];
      memcpy(desc2 + (size_t)j * 32, mpd + (size_t)j * 32, 32);
      desc2[(size_t)j * 32 + j % 32] ^= 0x11;
      planted += valid[j];
    }
  }
  in.n1 = n1; in.valid1 = valid; in.world_pos1 = wp; in.mp_desc1 = mpd; in.mp_observed1 = observed; in.octave1 = oct1; in.angle1 = ang1;
  in.n2 = n2; in.kp2_xy = xy2; in.kp2_octave = oct2; in.kp2_angle = ang2; in.uright2 = ur2; in.desc2 = desc2;
  in.grid[0] = 0; in.grid[1] = 0; in.grid[2] = W; in.grid[3] = H; in.grid[4] = 64.f / W; in.grid[5] = 48.f / H;
  in.Tcw_q[3] = 1.f; in.Tcw_t[0] = -tx; in.Tlw_q[3] = 1.f;
  in.K[0] = fx; in.K[1] = fy; in.K[2] = cx; in.K[3] = cy; in.mb = 0.08f; in.mbf = 40.f;
  in.scale_factors = sf; in.n_levels = levels; in.th = 7.f; in.mono = 0; in.check_orientation = 1;
  int32_t* match2 = heap<int32_t>(n2);
  int nm = 0, right = 0, outside = 0;
  CHECK(rgbl_search_by_projection(mt, &in, match2, &nm));
  for (int j = 0; j < n2; ++j) { outside += match2[j] < -1 || match2[j] >= n1; right += match2[j] == j; }
  printf("projection: %d matches, %d of %d planted ones, checksum %08x\n", nm, right, planted, sum_bytes(match2, 4 * n2));
  free(match2); free(sf); free(oct2); free(oct1); free(ur2); free(ang2); free(xy2); free(ang1); free(wp); free(desc2); free(mpd); free(observed); free(valid);
  return outside != 0 || right * 2 < planted;
}

static int run_sim3(rgbl_matcher* mt) {
  const int n = 65, n_hyp = 5;
  rgbl_sim3_input in;
  memset(&in, 0, sizeof(in));
  float *x1 = heap<float>((size_t)3 * n), *x2 = heap<float>((size_t)3 * n), *e1 = heap<float>(n), *e2 = heap<float>(n);
  int32_t* samples = heap<int32_t>((size_t)3 * n_hyp);
  const float c = std::cos(0.1f), s = std::sin(0.1f), scale = 1.1f;
  for (int i = 0; i < n; ++i) {
    const float z = 3.f + 10.f * unit(), x = (unit() - 0.5f) * z, y = (unit() - 0.5f) * z;
    x2[3 * i] = x; x2[3 * i + 1] = y; x2[3 * i + 2] = z;
    // x1 = s R x2 + t, every seventh point somewhere else
    x1[3 * i] = scale * (c * x + s * z) + 0.2f; x1[3 * i + 1] = scale * y - 0.1f; x1[3 * i + 2] = scale * (-s * x + c * z) + 0.3f;
    if (i % 7 == 3) x1[3 * i] += 1.5f;
    e1[i] = e2[i] = (float)(int)(9.210f * (1.f + (i % 3)));
  }
  for (int k = 0; k < n_hyp; ++k) { samples[3 * k] = (11 * k) % n; samples[3 * k + 1] = (11 * k + 20) % n; samples[3 * k + 2] = (11 * k + 41) % n; }
  in.n = n; in.x1c = x1; in.x2c = x2; in.max_err1 = e1; in.max_err2 = e2;
  in.K1[0] = in.K2[0] = 500.f; in.K1[1] = in.K2[1] = 500.f; in.K1[2] = in.K2[2] = 320.f; in.K1[3] = in.K2[3] = 240.f;
  in.fix_scale = 0; in.min_inliers = 20; in.best_inliers = 0; in.n_hyp = n_hyp; in.samples = samples;
  rgbl_sim3_output dev, host;
  memset(&dev, 0, sizeof(dev)); memset(&host, 0, sizeof(host));
  dev.inlier = heap<uint8_t>(n); host.inlier = heap<uint8_t>(n);
  dev.counts = heap<int32_t>(n_hyp); host.counts = heap<int32_t>(n_hyp);
  memset(dev.inlier, 0, n); memset(host.inlier, 0, n);
  CHECK(rgbl_sim3_ransac(mt, &in, &dev));
  CHECK(rgbl_sim3_ransac_host(&in, &host));
  const bool same = dev.selected == host.selected && dev.n_inliers == host.n_inliers && dev.iterations_run == host.iterations_run &&
                    !memcmp(dev.counts, host.counts, 4 * n_hyp) && (dev.selected < 0 || (!memcmp(dev.T12, host.T12, sizeof(dev.T12)) && !memcmp(dev.inlier, host.inlier, n)));
  printf("sim3: hypothesis %d with %d inliers, %s the host build, checksum %08x\n", dev.selected, dev.n_inliers, same ? "equal to" : "DIFFERS from",
         sum_bytes(dev.counts, 4 * n_hyp) ^ sum_bytes(dev.T12, sizeof(dev.T12)));
  free(host.counts); free(dev.counts); free(host.inlier); free(dev.inlier); free(samples); free(e2); free(e1); free(x2); free(x1);
  return !same || dev.selected < 0;
}

static int run_lba(rgbl_matcher* mt) {
  const int n_free = 2, n_fixed = 1, nc = n_free + n_fixed, np = 14, ne = np * nc;
  rgbl_lba_input in;
  memset(&in, 0, sizeof(in));
  float *q = heap<float>((size_t)4 * nc), *t = heap<float>((size_t)3 * nc), *K = heap<float>((size_t)4 * nc), *bf = heap<float>(nc);
  float *wp = heap<float>((size_t)3 * np), *obs = heap<float>((size_t)3 * ne), *is2 = heap<float>(ne);
  int32_t *ep = heap<int32_t>(ne), *ec = heap<int32_t>(ne);
  for (int c = 0; c < nc; ++c) {
    q[4 * c] = q[4 * c + 1] = q[4 * c + 2] = 0.f; q[4 * c + 3] = 1.f;
    t[3 * c] = -0.3f * c; t[3 * c + 1] = 0.02f * c; t[3 * c + 2] = 0.f;
    K[4 * c] = 500.f; K[4 * c + 1] = 500.f; K[4 * c + 2] = 320.f; K[4 * c + 3] = 240.f; bf[c] = 40.f;
  }
  for (int p = 0; p < np; ++p) { const float z = 4.f + 8.f * unit(); wp[3 * p] = (unit() - 0.5f) * z; wp[3 * p + 1] = (unit() - 0.5f) * z * 0.7f; wp[3 * p + 2] = z; }
  int e = 0;
  for (int p = 0; p < np; ++p)
    for (int c = 0; c < nc; ++c, ++e) {
      const float X = wp[3 * p] + t[3 * c], Y = wp[3 * p + 1] + t[3 * c + 1], Z = wp[3 * p + 2];
      ep[e] = p; ec[e] = c;
      obs[3 * e] = 500.f * X / Z + 320.f + (unit() - 0.5f); obs[3 * e + 1] = 500.f * Y / Z + 240.f + (unit() - 0.5f);
      obs[3 * e + 2] = (p + c) % 2 ? obs[3 * e] - 40.f / Z : -1.f;   // stereo and monocular edges mixed
      is2[e] = 1.f / (1.f + 0.44f * (e % 3));
    }
  in.n_free = n_free; in.n_fixed = n_fixed; in.cam_q = q; in.cam_t = t; in.cam_K = K; in.cam_bf = bf;
  in.n_points = np; in.world_pos = wp; in.n_edges = ne; in.edge_point = ep; in.edge_cam = ec; in.edge_obs = obs; in.edge_inv_sigma2 = is2;
  in.max_iterations = 10;
  rgbl_lba_output out[2];
  for (rgbl_lba_output& o : out) {
    memset(&o, 0, sizeof(o));
    o.cam_q = heap<float>((size_t)4 * n_free); o.cam_t = heap<float>((size_t)3 * n_free); o.point = heap<float>((size_t)3 * np);
    o.chi2 = heap<double>(ne); o.flags = heap<uint8_t>(ne);
  }
  CHECK(rgbl_local_bundle_adjustment(mt, &in, &out[0]));
  CHECK(rgbl_local_bundle_adjustment_host(&in, &out[1]));
  const bool same = out[0].diag.ran == out[1].diag.ran && out[0].diag.iterations == out[1].diag.iterations && out[0].diag.trials == out[1].diag.trials &&
                    !memcmp(out[0].cam_q, out[1].cam_q, 16 * n_free) && !memcmp(out[0].cam_t, out[1].cam_t, 12 * n_free) &&
                    !memcmp(out[0].point, out[1].point, 12 * np) && !memcmp(out[0].chi2, out[1].chi2, 8 * ne) && !memcmp(out[0].flags, out[1].flags, ne);
  printf("lba: %d iterations, %d trials, %s the host build, checksum %08x\n", out[0].diag.iterations, out[0].diag.trials, same ? "equal to" : "DIFFERS from",
         sum_bytes(out[0].point, 12 * np) ^ sum_bytes(out[0].chi2, 8 * ne));
  const int ran = out[0].diag.ran;
  for (rgbl_lba_output& o : out) { free(o.flags); free(o.chi2); free(o.point); free(o.cam_t); free(o.cam_q); }
  free(ec); free(ep); free(is2); free(obs); free(wp); free(bf); free(K); free(t); free(q);
  return !same || !ran;
}

static int child(const char* byte) {
  setenv("RGBL_ALLOC_FILL", byte, 1);   // before the first library call: the switch is read once per process
  printf("RGBL_ALLOC_FILL=%s\n", byte);
  if (run_extractor() || run_depth()) return 1;
  rgbl_matcher* mt = nullptr;
  CHECK(rgbl_matcher_create(0, &mt));
  // the LARGE layouts first, so that the small ones are carved out of what they left
  const int rc = run_hamming(mt) || run_projection(mt) || run_lba(mt) || run_sim3(mt) || run_projection(mt) || run_hamming(mt);
  rgbl_matcher_destroy(mt);
  if (!rc) printf("fill ok\n");
  fflush(stdout);
  return rc;
}

int main(int argc, char** argv) {
  if (argc > 1) return child(argv[1]);
  for (const char* byte : {"0xff", "0x5a"}) {
    fflush(stdout);
    const pid_t pid = fork();
    if (pid == 0) _exit(child(byte));
    int status = 0;
    if (pid < 0 || waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
      printf("the run with RGBL_ALLOC_FILL=%s failed (status %d)\n", byte, status);
      return 1;
    }
  }
  printf("bounds ok\n");
  return 0;
}
