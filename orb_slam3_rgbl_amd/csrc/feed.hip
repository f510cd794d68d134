// feed.hip — host-fed batches (include/rgbl_frontend.h: rgbl_feeder_*).
//
// The batched form of what one frame of Examples/RGB-L/rgbl_kitti.cc:87-94 costs the reference: Tracking::GrabImageRGBL
// (src/Tracking.cc:1563-1582: cvtColor) + Frame::Frame(imGray, PointCloud, ...) (src/Frame.cc:289-377: ExtractORB,
// UndistortKeyPoints, CalculateDepthFromPcd), for frames that arrive in host memory.  No kernel of its own: the slots' inputs
// go up on a copy stream, the existing kernels run on the handles' streams, events order the three.
//
// Per slot s (ring of `slots`), batch k:
//   copy stream      wait img_free[s], scan_free[s] (the batch k - slots readers) | H2D images | H2D scans | H2D offsets | in[s]
//   extractor stream wait in[s] | k_cvt_gray -> gray | extraction | img_free[s] | flag word -> slot, cleared | k_undistort |
//                    extracted[s]
//   depth stream     wait in[s] | varlen projection + up-sampling | scan_free[s] | overflow flag -> slot, cleared |
//                    wait extracted[s] | keypoint gather | D2H results (flags included) | done[s]
// The D2H sits behind the gather on the depth stream: on the copy stream it would hold the next batch's inputs back until this
// batch's kernels were done, and the ring would lose its overlap.
#include <string.h>

#include <algorithm>

#include "common.h"

using namespace rgbl;

namespace {
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// the results of one batch, the same layout on the device and in the page-locked block
struct OutLayout {
  size_t n, mono, flags, kp, desc, depth, uright, kpun, bytes;
  void init(int B, int cap, bool undist) {
    size_t o = 0;
    auto take = [&](size_t b) { const size_t at = o; o += align256(b); return at; };
    n = take(sizeof(int32_t) * B);
    mono = take(sizeof(int32_t) * B);
    flags = take(sizeof(int32_t) * 2);
    kp = take(sizeof(rgbl_keypoint) * (size_t)B * cap);
    desc = take((size_t)B * cap * 32);
    depth = take(sizeof(float) * (size_t)B * cap);
    uright = take(sizeof(float) * (size_t)B * cap);
    kpun = undist ? take(sizeof(float) * 2 * (size_t)B * cap) : 0;
    bytes = o;
  }
};
}  // namespace

struct rgbl_feeder {
  rgbl_feeder_cfg cfg;
  rgbl_extractor* ex = nullptr;
  rgbl_depth* dm = nullptr;
  int device = 0, w = 0, h = 0, cap = 0;
  bool undist = false;
  int* d_dm_err = nullptr;     // the depth handle's overflow flag
  size_t img_bytes = 0;        // one frame: w * h * channels
  size_t in_bytes = 0;         // images | scans | offsets of one slot
  size_t scan_at = 0, off_at = 0;
  OutLayout out;
  hipStream_t copy = nullptr;
  uint8_t* d_gray = nullptr;   // cvtColor's output, shared by the slots (the extractor stream orders its writers and readers)
  long long pinned = 0;
  int next = 0;
  // kFailed: a submit that returned an error after queueing part of its work; collect drains the streams and reports it
  enum { kIdle = 0, kFilling = 1, kSubmitted = 2, kFailed = 3 };
  struct Slot {
    int state = kIdle;
    int reserved = 0;          // frames whose scan is reserved
    int batch = 0;             // frames of the last submitted batch
    int max_n = 0;             // longest scan reserved
    int submit_rc = RGBL_OK;   // kFailed: what the submit returned
    uint8_t* h = nullptr;      // page-locked: inputs (in_bytes) | results (out.bytes)
    uint8_t* d = nullptr;      // device: the same
    hipEvent_t in = nullptr, img_free = nullptr, scan_free = nullptr, extracted = nullptr, done = nullptr;
  };
  std::vector<Slot> slot;
};

namespace {
int check_slot(rgbl_feeder* f, int slot) {
  if (!f) { set_error("null feeder"); return RGBL_ERR_INVALID; }
  if (slot < 0 || slot >= f->cfg.slots) { set_error("feeder slot %d out of range (%d slots)", slot, f->cfg.slots); return RGBL_ERR_INVALID; }
  return RGBL_OK;
}

void fill_results(const rgbl_feeder* f, const uint8_t* base, int batch, rgbl_feeder_results* r) {
  const OutLayout& o = f->out;
  r->batch = batch;
  r->cap = f->cap;
  r->kp = reinterpret_cast<const rgbl_keypoint*>(base + o.kp);
  r->desc = base + o.desc;
  r->n = reinterpret_cast<const int32_t*>(base + o.n);
  r->mono = reinterpret_cast<const int32_t*>(base + o.mono);
  r->depth = reinterpret_cast<const float*>(base + o.depth);
  r->uright = reinterpret_cast<const float*>(base + o.uright);
  r->kpun_xy = f->undist ? reinterpret_cast<const float*>(base + o.kpun) : nullptr;
}
}  // namespace

extern "C" {

int rgbl_feeder_create(const rgbl_feeder_cfg* cfg, rgbl_extractor* ex, rgbl_depth* dm, rgbl_feeder** out) {
  if (!cfg || !ex || !dm || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  int ew, eh, eb, dev, dw, dh, dp, db;
  int *ex_err, *dm_err;
  RGBL_TRY(rgbl_internal_extractor_info(ex, &ew, &eh, &eb, &dev, &ex_err));
  RGBL_TRY(rgbl_internal_depth_info(dm, &dw, &dh, &dp, &db, &dm_err));
  const long long pts_batch = cfg->max_points_batch ? cfg->max_points_batch : (long long)cfg->max_batch * cfg->max_points;
  const bool undist = cfg->n_dist > 0 && cfg->dist[0] != 0.0f;  // Frame.cc:839: nothing to undistort
  if ((cfg->channels != 1 && cfg->channels != 3 && cfg->channels != 4) || cfg->slots < 2 || cfg->max_batch < 1 ||
      cfg->max_batch > eb || cfg->max_batch > db || cfg->max_points < 0 || cfg->max_points > dp || pts_batch < 0 ||
      ew != dw || eh != dh || (cfg->n_dist != 0 && cfg->n_dist != 4 && cfg->n_dist != 5) ||
      (undist && (cfg->K[0] == 0.f || cfg->K[1] == 0.f))) {
    set_error("feeder configuration does not fit its handles (extractor %dx%d, batch %d; depth %dx%d, batch %d, %d points)", ew,
              eh, eb, dw, dh, db, dp);
    return RGBL_ERR_INVALID;
  }
  RGBL_HIP(hipSetDevice(dev));
  rgbl_feeder* f = new rgbl_feeder;
  f->cfg = *cfg;
  f->cfg.max_points_batch = pts_batch;
  f->ex = ex; f->dm = dm; f->device = dev; f->w = ew; f->h = eh;
  f->cap = rgbl_extractor_max_keypoints(ex);
  f->undist = undist;
  f->d_dm_err = dm_err;
  (void)ex_err;
  const size_t B = (size_t)cfg->max_batch;
  f->img_bytes = (size_t)ew * eh * cfg->channels;
  f->scan_at = align256(B * f->img_bytes + 64);   // + 64: k_cvt_gray's row loads may reach 16 bytes past the last pixel
  f->off_at = f->scan_at + align256(sizeof(float) * 4 * (size_t)pts_batch);
  f->in_bytes = f->off_at + align256(sizeof(int64_t) * (B + 1));
  f->out.init(cfg->max_batch, f->cap, undist);
  f->slot.resize(cfg->slots);
  int rc = RGBL_OK;
  auto fail = [&](const char* what) { set_error("feeder: %s failed", what); rc = RGBL_ERR_HIP; };
  if (hipStreamCreate(&f->copy) != hipSuccess) fail("hipStreamCreate");
  if (rc == RGBL_OK && cfg->channels != 1 && rgbl::device_alloc(&f->d_gray, B * ew * eh + 64) != hipSuccess) fail("hipMalloc");
  for (auto& s : f->slot) {
    if (rc != RGBL_OK) break;
    const size_t bytes = f->in_bytes + f->out.bytes;
    if (rgbl::pinned_alloc(&s.h, bytes) != hipSuccess) { s.h = nullptr; fail("hipHostMalloc"); break; }
    f->pinned += (long long)bytes;
    if (rgbl::device_alloc(&s.d, bytes) != hipSuccess) { s.d = nullptr; fail("hipMalloc"); break; }
    for (hipEvent_t* ev : {&s.in, &s.img_free, &s.scan_free, &s.extracted, &s.done})
      if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) { *ev = nullptr; fail("hipEventCreate"); break; }
  }
  if (rc != RGBL_OK) { rgbl_feeder_destroy(f); return rc; }
  *out = f;
  return RGBL_OK;
}

void rgbl_feeder_destroy(rgbl_feeder* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  bool failed = false;
  for (auto& s : f->slot) {
    if (s.state == rgbl_feeder::kSubmitted && s.done) (void)hipEventSynchronize(s.done);
    failed = failed || s.state == rgbl_feeder::kFailed;
  }
  if (failed) {  // part of a batch may be queued without its `done` event: drain the handles' streams
    (void)hipStreamSynchronize((hipStream_t)rgbl_extractor_stream(f->ex));
    (void)hipStreamSynchronize((hipStream_t)rgbl_depth_stream(f->dm));
  }
  if (f->copy) { (void)hipStreamSynchronize(f->copy); (void)hipStreamDestroy(f->copy); }
  for (auto& s : f->slot) {
    if (s.h) (void)hipHostFree(s.h);
    if (s.d) (void)hipFree(s.d);
    for (hipEvent_t ev : {s.in, s.img_free, s.scan_free, s.extracted, s.done})
      if (ev) (void)hipEventDestroy(ev);
  }
  if (f->d_gray) (void)hipFree(f->d_gray);
  delete f;
}

int rgbl_feeder_acquire(rgbl_feeder* f, int* slot) {
  if (!f || !slot) { set_error("null argument"); return RGBL_ERR_INVALID; }
  auto& s = f->slot[f->next];
  if (s.state == rgbl_feeder::kSubmitted || s.state == rgbl_feeder::kFailed) {
    set_error("feeder slot %d: its batch was submitted and not collected (collect it before acquiring the slot again)", f->next);
    return RGBL_ERR_INVALID;
  }
  if (s.state == rgbl_feeder::kFilling) { set_error("feeder slot %d is still being filled (submit it first)", f->next); return RGBL_ERR_INVALID; }
  s.state = rgbl_feeder::kFilling;
  s.reserved = 0;
  s.max_n = 0;
  reinterpret_cast<int64_t*>(s.h + f->off_at)[0] = 0;
  *slot = f->next;
  f->next = (f->next + 1) % f->cfg.slots;
  return RGBL_OK;
}

int rgbl_feeder_image(rgbl_feeder* f, int slot, int b, uint8_t** px) {
  RGBL_TRY(check_slot(f, slot));
  auto& s = f->slot[slot];
  if (!px || s.state != rgbl_feeder::kFilling || b < 0 || b >= f->cfg.max_batch) {
    set_error("feeder image: slot %d is not being filled, or frame %d is outside the batch (%d)", slot, b, f->cfg.max_batch);
    return RGBL_ERR_INVALID;
  }
  *px = s.h + (size_t)b * f->img_bytes;
  return RGBL_OK;
}

int rgbl_feeder_scan(rgbl_feeder* f, int slot, int b, int n, float** xyzi) {
  RGBL_TRY(check_slot(f, slot));
  auto& s = f->slot[slot];
  if (!xyzi || s.state != rgbl_feeder::kFilling || b != s.reserved || b >= f->cfg.max_batch || n < 0) {
    set_error("feeder scan: slot %d is not being filled, or frame %d is not the next one to reserve (%d)", slot, b, s.reserved);
    return RGBL_ERR_INVALID;
  }
  int64_t* off = reinterpret_cast<int64_t*>(s.h + f->off_at);
  if (n > f->cfg.max_points || off[b] + n > f->cfg.max_points_batch) {
    set_error("feeder scan: %d points for frame %d exceed the feeder's room (%d per scan, %lld per batch, %lld in use)", n, b,
              f->cfg.max_points, f->cfg.max_points_batch, (long long)off[b]);
    return RGBL_ERR_CAPACITY;
  }
  *xyzi = reinterpret_cast<float*>(s.h + f->scan_at) + 4 * (size_t)off[b];
  off[b + 1] = off[b] + n;
  s.max_n = std::max(s.max_n, n);
  ++s.reserved;
  return RGBL_OK;
}

}  // extern "C"

namespace {
// everything one batch queues (rgbl_feeder_submit); on an error return part of it may be queued already
int enqueue_batch(rgbl_feeder* f, rgbl_feeder::Slot& s, int batch) {
  RGBL_HIP(hipSetDevice(f->device));
  const int64_t used = reinterpret_cast<const int64_t*>(s.h + f->off_at)[batch];
  const size_t cap = (size_t)f->cap;
  hipStream_t cs = f->copy;
  hipStream_t es = (hipStream_t)rgbl_extractor_stream(f->ex);
  hipStream_t ds = (hipStream_t)rgbl_depth_stream(f->dm);
  // inputs: behind the device slot's last readers (batch k - slots; an event never recorded does not hold anything back)
  RGBL_HIP(hipStreamWaitEvent(cs, s.img_free, 0));
  RGBL_HIP(hipStreamWaitEvent(cs, s.scan_free, 0));
  RGBL_HIP(hipMemcpyAsync(s.d, s.h, (size_t)batch * f->img_bytes, hipMemcpyHostToDevice, cs));
  if (used > 0)
    RGBL_HIP(hipMemcpyAsync(s.d + f->scan_at, s.h + f->scan_at, sizeof(float) * 4 * (size_t)used, hipMemcpyHostToDevice, cs));
  RGBL_HIP(hipMemcpyAsync(s.d + f->off_at, s.h + f->off_at, sizeof(int64_t) * (batch + 1), hipMemcpyHostToDevice, cs));
  RGBL_HIP(hipEventRecord(s.in, cs));
  // extraction: GrabImageRGBL's cvtColor, ORBextractor::operator(), UndistortKeyPoints
  uint8_t* d_o = s.d + f->in_bytes;
  const OutLayout& o = f->out;
  auto* d_kp = reinterpret_cast<rgbl_keypoint*>(d_o + o.kp);
  auto* d_n = reinterpret_cast<int32_t*>(d_o + o.n);
  int32_t* d_flags = reinterpret_cast<int32_t*>(d_o + o.flags);
  RGBL_HIP(hipStreamWaitEvent(es, s.in, 0));
  const uint8_t* gray = s.d;
  if (f->cfg.channels != 1) {
    RGBL_TRY(rgbl_cvt_gray_batch_device(f->ex, s.d, batch, f->cfg.channels, f->cfg.blue_first, f->w, f->h, f->w * f->cfg.channels,
                                        f->img_bytes, f->d_gray, f->w, (size_t)f->w * f->h));
    gray = f->d_gray;
    RGBL_HIP(hipEventRecord(s.img_free, es));
  }
  RGBL_TRY(rgbl_extract_batch_device(f->ex, gray, batch, f->w, f->h, f->w, (size_t)f->w * f->h, 0, 0, d_kp, d_o + o.desc, (int)cap,
                                     d_n, reinterpret_cast<int32_t*>(d_o + o.mono)));
  if (f->cfg.channels == 1) RGBL_HIP(hipEventRecord(s.img_free, es));
  // the extractor's flag word of THIS batch: taken (and cleared) right behind its extraction, on the extractor's stream
  RGBL_TRY(rgbl_internal_extractor_take_flags(f->ex, d_flags));
  float* d_kpun = f->undist ? reinterpret_cast<float*>(d_o + o.kpun) : nullptr;
  if (f->undist)
    RGBL_TRY(rgbl_undistort_keypoints_batch_device(f->ex, d_kp, d_n, batch, (int)cap, f->cfg.K, f->cfg.dist, f->cfg.n_dist, d_kpun));
  RGBL_HIP(hipEventRecord(s.extracted, es));
  // depth: the projection runs next to the extraction, the gather waits for the keypoints
  RGBL_HIP(hipStreamWaitEvent(ds, s.in, 0));
  RGBL_TRY(rgbl_depth_project_xyzi_varlen_batch_device(f->dm, reinterpret_cast<const float*>(s.d + f->scan_at),
                                                       reinterpret_cast<const int64_t*>(s.d + f->off_at), batch, s.max_n, f->w,
                                                       f->h, nullptr));
  RGBL_HIP(hipEventRecord(s.scan_free, ds));
  // the depth handle's overflow flag of this batch, likewise (the depth stream orders it behind the projection)
  RGBL_HIP(hipMemcpyAsync(d_flags + 1, f->d_dm_err, sizeof(int32_t), hipMemcpyDeviceToDevice, ds));
  RGBL_HIP(hipMemsetAsync(f->d_dm_err, 0, sizeof(int32_t), ds));
  RGBL_HIP(hipStreamWaitEvent(ds, s.extracted, 0));
  float* d_depth = reinterpret_cast<float*>(d_o + o.depth);
  float* d_uright = reinterpret_cast<float*>(d_o + o.uright);
  if (f->undist) RGBL_TRY(rgbl_internal_depth_gather_xy(f->dm, batch, d_kp, d_n, (int)cap, d_kpun, d_depth, d_uright));
  else RGBL_TRY(rgbl_depth_gather_batch_device(f->dm, batch, f->w, f->h, d_kp, d_n, (int)cap, nullptr, d_depth, d_uright));
  // results home, behind the gather (never on the copy stream, see the top of the file): counts | mono | flags | keypoints in
  // one copy, then descriptors, depths, uRights, undistorted points
  uint8_t* h_o = s.h + f->in_bytes;
  RGBL_HIP(hipMemcpyAsync(h_o, d_o, o.kp + (size_t)batch * cap * sizeof(rgbl_keypoint), hipMemcpyDeviceToHost, ds));
  RGBL_HIP(hipMemcpyAsync(h_o + o.desc, d_o + o.desc, (size_t)batch * cap * 32, hipMemcpyDeviceToHost, ds));
  RGBL_HIP(hipMemcpyAsync(h_o + o.depth, d_o + o.depth, sizeof(float) * batch * cap, hipMemcpyDeviceToHost, ds));
  RGBL_HIP(hipMemcpyAsync(h_o + o.uright, d_o + o.uright, sizeof(float) * batch * cap, hipMemcpyDeviceToHost, ds));
  if (f->undist) RGBL_HIP(hipMemcpyAsync(h_o + o.kpun, d_o + o.kpun, sizeof(float) * 2 * batch * cap, hipMemcpyDeviceToHost, ds));
  RGBL_HIP(hipEventRecord(s.done, ds));
  return RGBL_OK;
}
}  // namespace

extern "C" {

int rgbl_feeder_submit(rgbl_feeder* f, int slot, int batch) {
  RGBL_TRY(check_slot(f, slot));
  auto& s = f->slot[slot];
  if (s.state != rgbl_feeder::kFilling || batch < 1 || batch > f->cfg.max_batch || s.reserved != batch) {
    set_error("feeder submit: slot %d is not being filled, or the batch of %d frames does not match the %d reserved scans (max %d)",
              slot, batch, s.reserved, f->cfg.max_batch);
    return RGBL_ERR_INVALID;
  }
  s.batch = batch;
  const int rc = enqueue_batch(f, s, batch);
  // kSubmitted only once `done` is recorded behind this batch; a submit that failed half-way leaves the slot to collect, which
  // reports the failure instead of handing out another batch's results
  s.state = rc == RGBL_OK ? rgbl_feeder::kSubmitted : rgbl_feeder::kFailed;
  s.submit_rc = rc;
  return rc;
}

int rgbl_feeder_collect(rgbl_feeder* f, int slot, rgbl_feeder_results* out) {
  RGBL_TRY(check_slot(f, slot));
  auto& s = f->slot[slot];
  if (s.state == rgbl_feeder::kFailed) {
    // whatever the failed submit queued must be done before the slot's memory is handed out again
    RGBL_HIP(hipSetDevice(f->device));
    RGBL_HIP(hipStreamSynchronize(f->copy));
    RGBL_TRY(rgbl_extractor_sync(f->ex));
    RGBL_TRY(rgbl_depth_sync(f->dm));
    s.state = rgbl_feeder::kIdle;
    s.batch = 0;
    set_error("feeder collect: the submit of slot %d failed (status %d); the batch has no results", slot, s.submit_rc);
    return s.submit_rc != RGBL_OK ? s.submit_rc : RGBL_ERR_HIP;
  }
  if (s.state != rgbl_feeder::kSubmitted) {
    set_error("feeder collect: slot %d holds no submitted batch (collected already?)", slot);
    return RGBL_ERR_INVALID;
  }
  RGBL_HIP(hipSetDevice(f->device));
  RGBL_HIP(hipEventSynchronize(s.done));
  s.state = rgbl_feeder::kIdle;
  const uint8_t* h_o = s.h + f->in_bytes;
  if (out) fill_results(f, h_o, s.batch, out);
  // the flags were taken behind this batch's own extraction and projection (and cleared there): they concern this batch only
  const int32_t* flags = reinterpret_cast<const int32_t*>(h_o + f->out.flags);
  if (flags[0] & 3) {
    set_error("feeder collect: quad-tree scratch overflow in this batch (flags=%d)", flags[0]);
    return RGBL_ERR_OVERFLOW;
  }
  if (flags[0]) {
    set_error("feeder collect: more keypoints than the capacity in this batch");
    return RGBL_ERR_CAPACITY;
  }
  if (flags[1]) {
    set_error("feeder collect: a scan of this batch held more points than the feeder's max_points");
    return RGBL_ERR_OVERFLOW;
  }
  return RGBL_OK;
}

int rgbl_feeder_device_outputs(rgbl_feeder* f, int slot, rgbl_feeder_results* out, void** done_event) {
  RGBL_TRY(check_slot(f, slot));
  auto& s = f->slot[slot];
  if (!out || s.batch < 1 || s.state == rgbl_feeder::kFilling || s.state == rgbl_feeder::kFailed) {
    set_error("feeder device outputs: slot %d holds no submitted batch", slot);
    return RGBL_ERR_INVALID;
  }
  fill_results(f, s.d + f->in_bytes, s.batch, out);
  if (done_event) *done_event = (void*)s.done;
  return RGBL_OK;
}

long long rgbl_feeder_pinned_bytes(const rgbl_feeder* f) { return f ? f->pinned : 0; }

}  // extern "C"
