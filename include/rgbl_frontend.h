/* rgbl_frontend.h — C ABI of librgbl_frontend.so: the MI355X-native RGB-L per-frame front end.
 *
 * This is the drop-in boundary for the hot path of TUMFTM/ORB_SLAM3_RGBL.  The reference has no FFI
 * layer; its boundary is the C++ class API of three classes, and each entry point below names the
 * reference interface it replaces (file:line under /root/reference).  The C++ shims in
 * orb_slam3_rgbl_amd/shim/ re-create those classes (same names, same signatures) on top of this ABI;
 * INTEGRATION.md shows the few lines a maintainer changes.
 *
 * Conventions
 *   - plain C types only; no C++/torch/HIP types in any signature (streams travel as void*).
 *   - every function returns an int status: RGBL_OK (0) or a negative RGBL_ERR_*; the message of the
 *     last failure on the calling thread is available from rgbl_last_error().  Nothing throws or aborts.
 *   - "host" entry points take host pointers, are synchronous and fill caller-owned buffers
 *     (capacity in, count out) — the contract of the reference classes.
 *   - "_device" entry points take device (HBM) pointers, only ENQUEUE work on the handle's stream and
 *     return immediately; results are valid after rgbl_*_sync().  They exist so that batches of
 *     independent frames stay resident in HBM between extract -> depth -> match.
 *   - a handle owns one HIP stream + scratch memory and is NOT re-entrant (like the reference objects:
 *     ORBextractor/DepthModule keep per-call state in members); different handles may be driven from
 *     different threads concurrently.  Matcher entry points are stateless apart from their handle.
 *   - there is NO CPU fallback: if no gfx950 device is usable, create() fails with RGBL_ERR_NO_DEVICE.
 */
#ifndef RGBL_FRONTEND_H
#define RGBL_FRONTEND_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
  RGBL_OK = 0,
  RGBL_ERR_INVALID = -1,   /* bad argument */
  RGBL_ERR_NO_DEVICE = -2, /* no usable HIP device */
  RGBL_ERR_HIP = -3,       /* a HIP runtime call failed */
  RGBL_ERR_CAPACITY = -4,  /* caller buffer too small; counts are still reported */
  RGBL_ERR_OVERFLOW = -5,  /* an internal scratch bound was exceeded (never silently truncated) */
  RGBL_ERR_EMPTY = -6,     /* empty image: mirrors ORBextractor::operator() returning -1 */
  RGBL_ERR_COMM = -7       /* RCCL could not be loaded, or one of its calls failed (rgbl_comm_*, rgbl_gather_*) */
};

const char* rgbl_last_error(void);
/* "hip:gfx950" for the product build.  (The CPU SIMT emulation used by the test-suite reports "emu".) */
const char* rgbl_backend(void);
int rgbl_device_count(void);

/* cv::KeyPoint binary layout (28 bytes): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} rgbl_keypoint;

/* ------------------------------------------------------------------------------------------------
 * ORBextractor            replaces include/ORBextractor.h:49-83, src/ORBextractor.cc:409-469,1086-1195
 * ---------------------------------------------------------------------------------------------- */
typedef struct rgbl_extractor rgbl_extractor;

typedef struct {
  int nfeatures;       /* ORBextractor.nFeatures: every level's share + 24 <= 65535 (positions in the quad-tree's node list travel in
                        * 16 bits; one level: nfeatures <= 65511), RGBL_ERR_INVALID beyond */
  float scale_factor;  /* ORBextractor.scaleFactor */
  int nlevels;         /* ORBextractor.nLevels (<= 16) */
  int ini_th_fast;     /* ORBextractor.iniThFAST   */
  int min_th_fast;     /* ORBextractor.minThFAST   */
  int width, height;   /* image size this handle is built for (64 .. 4096 each: a quad-tree node's x travels in 12 bits of its sort
                        * key; every level at least one 35-px detection cell and at most 16 quad-tree roots wide) */
  int max_batch;       /* frames per batched call (>= 1) */
} rgbl_extractor_cfg;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.h:49-50).  `device` = HIP device ordinal. */
int rgbl_extractor_create(const rgbl_extractor_cfg* cfg, int device, rgbl_extractor** out);
void rgbl_extractor_destroy(rgbl_extractor* h);

/* Getters GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (ORBextractor.h:61-81) plus mnFeaturesPerLevel and umax; any pointer may be NULL.
 * Arrays hold nlevels entries (umax16: 16). Computed exactly as ORBextractor.cc:414-468 (fp32). */
int rgbl_extractor_tables(const rgbl_extractor* h, float* scale, float* inv_scale, float* sigma2,
                          float* inv_sigma2, int* features_per_level, int* umax16);
/* Upper bound of keypoints one frame can produce (sum over levels of quota + slack). */
int rgbl_extractor_max_keypoints(const rgbl_extractor* h);

/* int ORBextractor::operator()(image, mask [ignored], keypoints, descriptors, vLappingArea)
 * (ORBextractor.h:57-59, ORBextractor.cc:1086-1168).  Host image CV_8UC1 w x h with `stride` bytes per
 * row; writes up to `cap` keypoints and cap x 32 descriptor bytes, *out_n = number of keypoints,
 * *out_mono = the reference's return value (monoIndex).  Empty image -> RGBL_ERR_EMPTY, *out_mono=-1. */
int rgbl_extract(rgbl_extractor* h, const uint8_t* img, int w, int h_, int stride, int lap0, int lap1,
                 rgbl_keypoint* out_kp, uint8_t* out_desc, int cap, int* out_n, int* out_mono);
/* Latency of one frame (optional): the upload of the image, the whole extraction and the copies of its results into the
 * handle's page-locked block are queued and NOT waited for.  The rgbl_extract call that follows with the same image pointer,
 * size, stride and lapping area collects the results (any other extraction call waits for the begun one and drops it).  Work
 * queued on other handles in between - rgbl_depth_prefetch above all - runs next to the extraction, and so does the host.
 * The image must stay unchanged until it is collected. */
int rgbl_extract_begin(rgbl_extractor* h, const uint8_t* img, int w, int h_, int stride, int lap0, int lap1);
/* Drops a begun extraction that will not be collected (waits for it, forgets it).  A begun frame is recognised by its host
 * pointer, size, stride and lapping area alone: call this before freeing a buffer that was begun but never handed to
 * rgbl_extract - an allocator may give the address to the next frame, which would then collect the old frame's results. */
int rgbl_extract_cancel(rgbl_extractor* h);

/* Batched host variant: `batch` images of identical size, image b at imgs + b*frame_stride bytes.
 * Outputs for frame b start at out_kp + b*cap and out_desc + b*cap*32; out_n/out_mono hold batch ints. */
int rgbl_extract_batch(rgbl_extractor* h, const uint8_t* imgs, int batch, int w, int h_, int stride,
                       size_t frame_stride, int lap0, int lap1, rgbl_keypoint* out_kp,
                       uint8_t* out_desc, int cap, int* out_n, int* out_mono);

/* Device-resident batch: d_imgs / d_kp / d_desc / d_n / d_mono are device pointers with the same
 * layout as above (d_n, d_mono: int32[batch]).  Enqueues only; keypoints beyond `cap` are dropped and
 * flagged: rgbl_extractor_sync() then returns RGBL_ERR_CAPACITY. */
int rgbl_extract_batch_device(rgbl_extractor* h, const uint8_t* d_imgs, int batch, int w, int h_,
                              int stride, size_t frame_stride, int lap0, int lap1, rgbl_keypoint* d_kp,
                              uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono);
/* Waits for the handle's stream and reports deferred device-side errors (overflow flags). */
int rgbl_extractor_sync(rgbl_extractor* h);

/* Ingest in front of the extractor: the cv::cvtColor of Tracking::GrabImageRGBL
 * (src/Tracking.cc:1567-1580; also GrabImageStereo / GrabImageMonocular :1469-1556).  8-bit, 3 or 4 interleaved channels
 * -> gray with OpenCV 4.x' fixed-point weights (R 9798, G 19235, B 3735, 15 bits, + 2^14 before the shift).
 * blue_first = 1 is COLOR_BGR2GRAY / COLOR_BGRA2GRAY (settings `Camera.RGB: 0`), 0 is COLOR_RGB2GRAY / COLOR_RGBA2GRAY.
 * Device variant: enqueued on the extractor's stream, so a following rgbl_extract_batch_device() on d_gray is ordered
 * behind it; frame b at d_src + b*src_frame_stride / d_gray + b*gray_frame_stride (bytes). */
int rgbl_cvt_gray_batch_device(rgbl_extractor* h, const uint8_t* d_src, int batch, int channels, int blue_first, int w,
                               int h_, int src_stride, size_t src_frame_stride, uint8_t* d_gray, int gray_stride,
                               size_t gray_frame_stride);
/* cvtColor + operator() in one call on a host colour image (channels 1 = already gray: plain rgbl_extract).
 * out_gray (nullable, gray_stride bytes per row) receives mImGray, which Tracking keeps for the viewer. */
int rgbl_extract_color(rgbl_extractor* h, const uint8_t* img, int channels, int blue_first, int w, int h_, int stride,
                       int lap0, int lap1, rgbl_keypoint* out_kp, uint8_t* out_desc, int cap, int* out_n, int* out_mono,
                       uint8_t* out_gray, int gray_stride);

/* Stereo rectification in front of cvtColor: the two cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) calls of
 * System::TrackStereo (src/System.cc:260-268; the maps are Settings::precomputeRectificationMaps' M1l/M2l and M1r/M2r,
 * src/Settings.cc:485-520, which the host keeps computing).  8-bit, 1, 3 or 4 interleaved channels, two CV_32FC1 maps of
 * the destination's size, BORDER_CONSTANT 0.  Restated from OpenCV 4.x (parity vs the restatement, unpinned):
 * sx = cvRound(map_x * 32) (fp32 product, half-to-even; NaN and |v| >= 2^31 give INT32_MIN), ix = saturate_cast<short>(sx >> 5),
 * fx = sx & 31, likewise y; dst = (sum of the four taps times (32 - fx | fx) * (32 - fy | fy) + 512) >> 10, a tap outside the
 * source counts as 0.
 * rgbl_rectifier_create (System.cc:260-268) reads the host maps (row y at map + y*map_stride_floats) ONCE, turns them
 * into fixed-point entries per 64 x 32 destination tile and uploads them; no later call allocates.  Sides 1 .. 16384. */
typedef struct rgbl_rectifier rgbl_rectifier;
int rgbl_rectifier_create(int device, int src_w, int src_h, int dst_w, int dst_h, const float* map_x, const float* map_y,
                          int map_stride_floats, rgbl_rectifier** out);
void rgbl_rectifier_destroy(rgbl_rectifier* r);
/* Sizes, how many destination tiles take the LDS-staged kernel and how many the direct (per-tap gather) one, and the bytes
 * of map storage on the device (System.cc:260-268 keeps 8 bytes of float map per pixel).  Any pointer may be NULL. */
int rgbl_rectifier_info(const rgbl_rectifier* r, int* src_w, int* src_h, int* dst_w, int* dst_h, int* staged_tiles,
                        int* direct_tiles, long long* map_bytes);
/* cv::remap (System.cc:260-268) of `batch` device-resident frames: frame b at d_src + b*src_frame_stride /
 * d_dst + b*dst_frame_stride (bytes).  Enqueued on the extractor's stream, so a following rgbl_cvt_gray_batch_device() or
 * rgbl_extract_batch_device() of that handle is ordered behind it. */
int rgbl_remap_batch_device(rgbl_rectifier* r, rgbl_extractor* h, const uint8_t* d_src, int batch, int channels,
                            int src_stride, size_t src_frame_stride, uint8_t* d_dst, int dst_stride, size_t dst_frame_stride);
/* cv::remap (System.cc:260-268) of one host image into a host image (imLeftRect / imRightRect), synchronous. */
int rgbl_remap(rgbl_rectifier* r, const uint8_t* src, int channels, int src_stride, uint8_t* dst, int dst_stride);
/* remap (System.cc:260-268) + cvtColor + operator() on one RAW host image: one upload, then rectification, the gray
 * conversion when channels > 1, and the extraction.  The rectifier's source size must be src_w x src_h and its destination
 * size the extractor's width x height (RGBL_ERR_INVALID otherwise).  out_gray (nullable) receives the rectified gray
 * image, which Tracking keeps as mImGray. */
int rgbl_extract_rectified(rgbl_extractor* h, rgbl_rectifier* r, const uint8_t* img, int channels, int blue_first, int src_w,
                           int src_h, int stride, int lap0, int lap1, rgbl_keypoint* out_kp, uint8_t* out_desc, int cap,
                           int* out_n, int* out_mono, uint8_t* out_gray, int gray_stride);

/* The image resize in front of cvtColor: cv::resize(im, imToFeed, settings_->newImSize()) that every System::Track* entry
 * makes when the settings file carries Camera.newWidth / Camera.newHeight (src/System.cc:269-271, 349-351, 486-489, 557-560;
 * the reference's EuRoC settings: 752 x 480 -> 600 x 350).  8-bit, 1, 3 or 4 interleaved channels, the default INTER_LINEAR, any
 * ratio on either axis, sides 1 .. 16384.  Restated from OpenCV 4.x (parity vs the restatement = the oracle's cv::resize at one
 * channel, unpinned): per axis f = (float)((d + 0.5) * scale - 0.5) with scale = 1.0 / ((double)dsize / ssize), s = floor(f),
 * f -= s, on x s < 0 -> (0, 0) and s >= sw - 1 -> (sw - 1, 0), rows s and s + 1 clamped into the image, weights
 * cvRound((1 - f) * 2048) and cvRound(f * 2048), dst = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2 with
 * h = p0 * a0 + p1 * a1, every channel on its own.  At exactly half size OpenCV takes INTER_AREA instead, which on 8-bit
 * images is the same number ((a + b + c + d + 2) >> 2), so one kernel serves both.  The depth map's resize of TrackRGBD
 * (System.cc:354, 425: CV_32F / CV_16U) stays on the host.
 * rgbl_resizer_create (System.cc:269-271, 349-351, 486-489, 557-560) builds the coefficient tables of both axes and the row
 * spans of the destination tiles ONCE and uploads them. */
typedef struct rgbl_resizer rgbl_resizer;
int rgbl_resizer_create(int device, int src_w, int src_h, int dst_w, int dst_h, rgbl_resizer** out);
void rgbl_resizer_destroy(rgbl_resizer* r);
/* Sizes, whether OpenCV would reroute this pair of sizes to INTER_AREA (System.cc:269-271, 349-351, 486-489, 557-560 at exactly
 * half size; the output is the same), and the bytes of tables on the device.  Any pointer may be NULL. */
int rgbl_resizer_info(const rgbl_resizer* r, int* src_w, int* src_h, int* dst_w, int* dst_h,
                      int* area_fast /* 1 when OpenCV would reroute to INTER_AREA */, long long* table_bytes);
/* cv::resize (System.cc:269-271, 349-351, 486-489, 557-560) of `batch` device-resident frames: frame b at
 * d_src + b*src_frame_stride / d_dst + b*dst_frame_stride (bytes), batch <= the extractor's max_batch.  Enqueued on the
 * extractor's stream, so a following rgbl_cvt_gray_batch_device() or rgbl_extract_batch_device() of that handle is ordered
 * behind it. */
int rgbl_resize_batch_device(rgbl_resizer* r, rgbl_extractor* h, const uint8_t* d_src, int batch, int channels, int src_stride,
                             size_t src_frame_stride, uint8_t* d_dst, int dst_stride, size_t dst_frame_stride);
/* cv::resize (System.cc:269-271, 349-351, 486-489, 557-560) of one host image into a host image (imToFeed), synchronous. */
int rgbl_resize(rgbl_resizer* r, const uint8_t* src, int channels, int src_stride, uint8_t* dst, int dst_stride);
/* resize (System.cc:269-271, 349-351, 486-489, 557-560) + cvtColor + operator() on one RAW host image: one upload, then the
 * resize AT THE IMAGE'S CHANNEL COUNT, the gray conversion when channels > 1, and the extraction - the reference's order
 * (System resizes the colour image, Tracking converts afterwards; gray-then-resize gives other bits).  The resizer's source
 * size must be src_w x src_h and its destination size the extractor's width x height (RGBL_ERR_INVALID otherwise).
 * out_gray (nullable) receives mImGray. */
int rgbl_extract_resized(rgbl_extractor* h, rgbl_resizer* r, const uint8_t* img, int channels, int blue_first, int src_w,
                         int src_h, int stride, int lap0, int lap1, rgbl_keypoint* out_kp, uint8_t* out_desc, int cap,
                         int* out_n, int* out_mono, uint8_t* out_gray, int gray_stride);

/* Frame::UndistortKeyPoints / the corner undistortion of Frame::ComputeImageBounds (src/Frame.cc:837-870, 872-900):
 * cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), mK) - normalise, OpenCV's 5 fixed-point iterations of the inverse
 * Brown-Conrady model in double, re-project with the same K.  K = fx, fy, cx, cy; dist = k1, k2, p1, p2[, k3] (n_dist 4 or 5).
 * SURVEY.md 8(f) row f3.  The reference skips the call when mDistCoef[0] == 0 (the KITTI settings); the shim keeps that test.
 * Host pointers, synchronous: n (x, y) pairs in, n pairs out (in place allowed). */
int rgbl_undistort_points(rgbl_extractor* h, const float* xy, int n, const float K[4], const float* dist, int n_dist, float* out_xy);
/* The keypoints of rgbl_extract_batch_device() (frame b at d_kp + b*cap, d_n counts) -> their undistorted coordinates,
 * d_xy_un[b][i] = (x, y) as 2 floats (cap pairs per frame); enqueued on the handle's stream. */
int rgbl_undistort_keypoints_batch_device(rgbl_extractor* h, const rgbl_keypoint* d_kp, const int32_t* d_n, int batch, int cap,
                                          const float K[4], const float* dist, int n_dist, float* d_xy_un);

/* std::vector<cv::Mat> mvImagePyramid (ORBextractor.h:83; read by Frame::ComputeStereoMatches,
 * Frame.cc:908,998-1013).  Copies level `level` of frame `frame` of the LAST call to host memory.
 * with_border=1 adds the 19-px BORDER_REFLECT_101 frame the reference keeps around every level
 * (ORBextractor.cc:1185-1191): dst is then (w+38) x (h+38).  blurred=1 returns the 7x7 Gaussian
 * working image of ORBextractor.cc:1132-1133 instead (no border). */
int rgbl_extractor_level_size(const rgbl_extractor* h, int level, int* w, int* h_);
int rgbl_extractor_get_level(rgbl_extractor* h, int frame, int level, int blurred, int with_border,
                             uint8_t* dst, int dst_stride);
/* Test/diagnostic access to the stage between FAST and the quad-tree: the candidates handed to
 * DistributeOctTree for (frame, level) in the reference's order, coordinates relative to minBorder
 * (ORBextractor.cc:863-868).  Returns the count through *out_n. */
int rgbl_extractor_get_candidates(rgbl_extractor* h, int frame, int level, rgbl_keypoint* out, int cap,
                                  int* out_n);

/* void Frame::ComputeStereoMatches() (src/Frame.cc:901-1071): for every left keypoint the best
 * right keypoint in its row band (Hamming, strict '<', octave +-1, disparity window from mb / mbf), 11x11 SAD
 * sub-pixel refinement over 11 shifts on the left keypoint's pyramid level, parabola fit, median*2.1 outlier cut.
 * `left` / `right` are the two extractor handles whose LAST extract call processed the left / right image(s): their
 * resident pyramids are read directly (the reference reads mpORBextractor{Left,Right}->mvImagePyramid), so the stereo
 * path needs no pyramid download.  Outputs mvuRight / mvDepth (-1 = no match).
 * Host variant: frame 0 of the last call, host arrays, synchronous.  Device variant: the layout of
 * rgbl_extract_batch_device() for both sides (frame b at + b*cap), enqueued on the left handle's stream.
 * At most 65535 keypoints per view: n_left, n_right and cap above that are refused with RGBL_ERR_INVALID; the per-frame counts must not exceed cap.
 * Every octave must lie in 0 .. nlevels - 1: the host variant refuses the call otherwise; the device variant cannot look at device data, so there this is the caller's contract. */
int rgbl_stereo_matches(rgbl_extractor* left, rgbl_extractor* right, const rgbl_keypoint* kp_left,
                        const uint8_t* desc_left, int n_left, const rgbl_keypoint* kp_right,
                        const uint8_t* desc_right, int n_right, float mb, float mbf, float* out_uright,
                        float* out_depth);
int rgbl_stereo_matches_batch_device(rgbl_extractor* left, rgbl_extractor* right, int batch,
                                     const rgbl_keypoint* d_kp_left, const uint8_t* d_desc_left,
                                     const int32_t* d_n_left, const rgbl_keypoint* d_kp_right,
                                     const uint8_t* d_desc_right, const int32_t* d_n_right, int cap, float mb,
                                     float mbf, float* d_uright, float* d_depth);

/* Diagnostics: with RGBL_OCTREE_STAMPS set in the environment the quad-tree kernel leaves 16 cycle-counter stamps
 * per (frame, level) workgroup; this copies them out. */
int rgbl_extractor_debug_stamps(rgbl_extractor* h, unsigned long long* out, int count);

/* Self-test on the device: the hand-written instruction wrappers of the kernels (v_mul_u32_u24 with a scalar operand,
 * v_addc_co_u32 with an SGPR mask, global_load_lds_dwordx4 from unaligned sources) against their plain expressions on n
 * random inputs in partially active waves.  RGBL_OK, or RGBL_ERR_HIP with the first mismatch in rgbl_last_error(). */
int rgbl_selftest_wrappers(int device, int n, unsigned seed);

/* Stream control + per-kernel timing (HIP events on the launch stream) for bench.py. */
int rgbl_extractor_set_stream(rgbl_extractor* h, void* hip_stream /* hipStream_t, NULL = own */);
void* rgbl_extractor_stream(rgbl_extractor* h); /* hipStream_t currently used by the handle */
/* the handle's second, internal stream (level-0 FAST / quad-tree and the Gaussian run there next to the resize chain);
 * other handles may queue work behind it with rgbl_*_set_stream */
void* rgbl_extractor_aux_stream(rgbl_extractor* h);
/* Device-side ordering between handles without a host sync: work enqueued on `waiter_stream` after this call
 * starts only when everything enqueued on `signaler_stream` before this call has finished (HIP event). */
int rgbl_stream_wait(void* waiter_stream, void* signaler_stream);
/* Multi-GPU gather, SURVEY.md 8(e): compacts a batch's per-frame results (device arrays as the batch entry points produce
 * them: counts, cap keypoints / descriptors / depths / uRights per frame) into variable-length records of 68 bytes per
 * keypoint (28 B cv::KeyPoint | 32 B descriptor | f32 depth | f32 uRight), frames back to back starting at record
 * `first_record` of d_out (which holds capacity_records records).  d_offsets[f] = first record of frame f,
 * d_offsets[batch] = one past the last; *d_overflow is set to 1 (and the frame skipped) when the records do not fit.
 * Enqueued on `hip_stream`, no host synchronisation.  There is no counterpart in the reference (it runs on one CPU). */
int rgbl_pack_records_device(void* hip_stream, const int32_t* d_n, const rgbl_keypoint* d_kp, const uint8_t* d_desc,
                             const float* d_depth, const float* d_uright, int batch, int cap, long long first_record,
                             long long capacity_records, uint8_t* d_out, long long* d_offsets, int* d_overflow);
/* ---- The gather itself, over RCCL (round 4).  `north_star`: "host stays C++ calling through a thin C-ABI ... RCCL over xGMI
 * only for the final keypoint/descriptor gather".  The reference has no counterpart (one process, one CPU); a multi-GPU host
 * loop in the style of Examples/RGB-L/rgbl_kitti.cc:87-125 (one process per GPU, each tracking its own sequences) calls:
 *
 *   rank 0:  rgbl_comm_unique_id(id);  -> id reaches the other ranks out of band (file, socket, MPI_Bcast, a torch store)
 *   all:     rgbl_comm_create(id, world, rank, device, &comm);            ncclCommInitRank
 *            rgbl_gather_create(comm, device, batch, cap, slots, stream, &g);
 *   per step k (slot = k % slots), behind the step's kernels, nothing waits on the host:
 *            rgbl_gather_pack(g, slot, d_n, d_kp, d_desc, d_depth, d_uright, wait_events, n, done_event);
 *                 pack (rgbl_pack_records_device) + phase 1: ncclAllGather of the per-frame counts of every rank, their copy into
 *                 page-locked host memory, an event behind it
 *   one step later (or all slots at the end: "final" gather):
 *            rgbl_gather_exchange(g, slot);
 *                 phase 2: the host waits for THAT slot's counts only and posts one exact-size ncclSend (non-root) resp. one
 *                 ncclRecv per peer (root) inside one ncclGroup - on MI355X one xGMI link per peer, in parallel
 *   root:    rgbl_gather_sync(g); rgbl_gather_result(g, r, &counts, &d_records, &n) for r = 0 .. world - 1
 *            The root owns TWO receive banks, used alternately: what rgbl_gather_result hands out is overwritten by the SECOND
 *            following rgbl_gather_exchange.  A gather at the end that exchanges several slots in a row must copy every
 *            exchange's records out (rgbl_gather_copy_result, queued on the gather's stream) before the exchange after next.
 *   Errors:  a slot is packed once and exchanged once, in that order (RGBL_ERR_INVALID otherwise - a rank that packed over a
 *            step it never exchanged would be one all-gather ahead of its peers).  An exchange that fails after some transfers
 *            were posted aborts the communicator (ncclCommAbort: the peers' matching calls return with an error instead of
 *            hanging) and the gather handle answers RGBL_ERR_COMM from then on.  rgbl_comm_destroy while gather handles still
 *            use the communicator is deferred to the last rgbl_gather_destroy.
 *
 * Everything is queued on ONE stream the library controls (default: a low-priority stream of its own; or the caller's, e.g. the
 * low-priority stream of the Hamming scan): the collectives do not get a stream of their own the way a framework's process group
 * gives them one.  librccl is loaded lazily (dlopen; an RCCL already mapped into the process - PyTorch's - is reused): a
 * single-GPU process never touches it; rgbl_comm_unique_id / rgbl_comm_create return RGBL_ERR_COMM if it cannot be loaded.
 * comm == NULL in rgbl_gather_create: one rank without RCCL (device copies), the same choreography. */
#define RGBL_COMM_ID_BYTES 128
typedef struct rgbl_comm rgbl_comm;
typedef struct rgbl_gather rgbl_gather;
int rgbl_comm_available(void);                                  /* 1 when an RCCL library can be loaded (loads it) */
int rgbl_comm_unique_id(uint8_t id[RGBL_COMM_ID_BYTES]);        /* ncclGetUniqueId */
int rgbl_comm_create(const uint8_t id[RGBL_COMM_ID_BYTES], int world, int rank, int device, rgbl_comm** out);
void rgbl_comm_destroy(rgbl_comm* c);   /* while gather handles use the communicator it lives on until the last of them is
                                            destroyed; a second call is valid only during that time (afterwards the object is gone) */
int rgbl_comm_info(const rgbl_comm* c, int* world, int* rank, int* device, int* rccl_version);
/* batch frames per step, cap keypoints per frame (the layout of the batch entry points' outputs), slots packed steps that
 * may wait for their exchange (2 = streaming, one step of slack; the number of steps for a gather at the end). */
int rgbl_gather_create(rgbl_comm* comm, int device, int batch, int cap, int slots, void* hip_stream, rgbl_gather** out);
void rgbl_gather_destroy(rgbl_gather* g);
void* rgbl_gather_stream(rgbl_gather* g);
/* one rank only: the root's own records travel through ncclSend / ncclRecv to itself instead of a device copy, so that a
 * one-GPU box exercises the point-to-point path (needs a comm) */
int rgbl_gather_set_loopback(rgbl_gather* g, int enable);
int rgbl_gather_pack(rgbl_gather* g, int slot, const int32_t* d_n, const rgbl_keypoint* d_kp, const uint8_t* d_desc,
                     const float* d_depth, const float* d_uright, void* const* wait_events, int n_wait, void* done_event);
int rgbl_gather_exchange(rgbl_gather* g, int slot);
int rgbl_gather_sync(rgbl_gather* g);   /* waits for the stream; RGBL_ERR_OVERFLOW if a pack did not fit its slot */
/* root, after rgbl_gather_exchange: the records of `rank` of the most recent exchange (valid until the exchange after the
 * next one: two receive banks) and their per-frame counts (host memory, `batch` ints).  The device pointer may be used by
 * work queued on rgbl_gather_stream, or after rgbl_gather_sync. */
int rgbl_gather_result(rgbl_gather* g, int rank, const int32_t** h_counts, const uint8_t** d_records, long long* n_records);
/* convenience: queues a copy of those records into dst (device or host memory, >= n_records * 68 bytes) on the gather's stream */
int rgbl_gather_copy_result(rgbl_gather* g, int rank, void* dst, long long capacity_bytes);
/* The same with explicit, reusable HIP events: record marks a point on a stream, wait makes later work on another
 * stream start only after that point (a never-recorded event does not block). Enables software pipelining across
 * batches: e.g. the extractor may overwrite an output buffer as soon as the event recorded behind its last reader
 * has fired, while the matcher still works on the other buffer. */
int rgbl_event_create(void** out_event);
void rgbl_event_destroy(void* event);
int rgbl_event_record(void* event, void* stream);
int rgbl_event_wait(void* stream, void* event);
/* A stream of the library's device with the lowest (priority < 0), the default (0) or the highest (> 0) scheduling priority,
 * to be handed to the rgbl_*_set_stream calls.  Work that is not on a batch pipeline's critical chain (the Hamming scan of
 * step k next to the extraction of step k + 1) belongs on a low-priority stream: its workgroups fill the slots the chain
 * leaves instead of competing for them (bench.py: +4 %). */
int rgbl_stream_create(void** out_stream, int priority);        /* on the calling thread's current device */
int rgbl_stream_create_on(int device, void** out_stream, int priority); /* on `device` (hipSetDevice first): what multi-GPU hosts call */
void rgbl_stream_destroy(void* stream);
int rgbl_extractor_profile(rgbl_extractor* h, int enable);
/* Returns the number of distinct kernels; fills up to cap entries. names[i] points to static storage. */
int rgbl_extractor_profile_read(rgbl_extractor* h, const char** names, double* total_ms, long* launches,
                                int cap);
/* Every launch's own duration (ms, launch order) of kernel number `kernel` (its index in rgbl_*_profile_read's arrays) since
 * profiling was switched on: returns how many there are, copies the first `cap`.  bench.py builds its per-step median /
 * min / max table from these without synchronising between steps (a host sync per step lets the GPU run dry, and the
 * event bracket of the first launches then measures the host's launch latency). */
int rgbl_extractor_profile_samples(rgbl_extractor* h, int kernel, float* ms, int cap);

/* ------------------------------------------------------------------------------------------------
 * DepthModule             replaces include/DepthModule.h:45-99, src/DepthModule.cc:50-274
 * ---------------------------------------------------------------------------------------------- */
typedef struct rgbl_depth rgbl_depth;

enum { /* DepthModule::UpsamlingMethod (DepthModule.h:34-40) */
  RGBL_UPS_NONE = 0,
  RGBL_UPS_NEAREST_NEIGHBOR_PIXEL = 1,
  RGBL_UPS_AVERAGE_FILTERING = 2,
  RGBL_UPS_INVERSE_DILATION = 3,
  RGBL_UPS_IPBASIC = 5 /* declared by the reference but never implemented: rejected here too */
};

typedef struct {
  float proj[12];      /* LidarProjectionMatrix = K[3x4] * Tr[4x4] (DepthModule.cc:434), row-major */
  float min_dist;      /* LiDAR.min_dist */
  float max_dist;      /* LiDAR.max_dist */
  float mbf;           /* Camera.bf */
  int method;          /* RGBL_UPS_* */
  int kernel_w, kernel_h;  /* inverse-dilation structuring element (<= 9 x 9), anchor = centre */
  uint8_t kernel[81];      /* row-major mask; see rgbl_structuring_element() */
  int avg_kernel_size;     /* LiDAR.MethodAverageFiltering.KernelSize */
  float nn_search_radius;  /* LiDAR.MethodNearestNeighborPixel.SearchDistance */
  int width, height;       /* image size */
  int max_points;          /* capacity for LiDAR points per scan (reference cap: 250000) */
  int max_keypoints;       /* capacity for keypoints per frame */
  int max_batch;
} rgbl_depth_cfg;

/* DepthModule::DepthModule(yaml, sensor) minus the YAML parsing (that stays in the C++ shim). */
int rgbl_depth_create(const rgbl_depth_cfg* cfg, int device, rgbl_depth** out);
void rgbl_depth_destroy(rgbl_depth* h);
/* LidarProjectionMatrix = CameraMatrix * RotationMatrix with OpenCV GEMM arithmetic (host helper). */
void rgbl_projection_matrix(const float K3x4[12], const float Tr4x4[16], float out3x4[12]);
/* cv::getStructuringElement (shape 0 RECT, 1 CROSS, 2 ELLIPSE) and the reference's Diamond tables
 * (shape 3, DepthModule.h:138-161; only kw is used).  out holds kh*kw bytes. */
int rgbl_structuring_element(int shape, int kw, int kh, uint8_t* out);

/* void DepthModule::CalculateDepthFromPcd(mvKeys, mvKeysUn, PointCloud, imwidth, imheight)
 * (DepthModule.h:62, DepthModule.cc:50-79).  cloud = the 4 x n CV_32F matrix of
 * Examples/RGB-L/rgbl_kitti.cc:151-185 (rows x,y,z,1; `ld` floats between rows).  kp_xy = k pairs
 * (pt.x, pt.y) of mvKeys, kpun_x = pt.x of mvKeysUn.  Outputs mvDepth / mvuRight (k floats each) and,
 * if non-NULL, RawDepthMap / ProcessedDepthMap (h*w floats each).
 * Any n up to max_points is taken.  Inverse dilation without the maps reads the points' depths through the index map, whose
 * entries are generation << 20 | point index + 1: scans of up to 2^20 - 2 points; from 2^20 - 1 points on the call goes through
 * the raw map as if the maps had been asked for (same results). */
int rgbl_depth_compute(rgbl_depth* h, const float* cloud, int n, int ld, int w, int h_,
                       const float* kp_xy, const float* kpun_x, int k, float* out_depth,
                       float* out_uright, float* out_raw, float* out_processed);

/* Latency of one frame (optional): the part of CalculateDepthFromPcd that does not depend on the keypoints - upload of the scan,
 * ProjectPointcloudToImage, the up-sampling (DepthModule.cc:57-76 without GetFeatureDepthFromDepthMap) - queued on the handle's
 * stream, not waited for.  Called between rgbl_extract_begin and rgbl_extract it runs next to the extraction; the
 * rgbl_depth_compute / _xyzi call that follows with the same cloud pointer, n and ld then only gathers the keypoints' depths
 * (with out_raw != NULL, or another cloud, it computes everything as usual).  The scan must stay unchanged in between. */
int rgbl_depth_prefetch(rgbl_depth* h, const float* cloud, int n, int ld, int w, int h_);
int rgbl_depth_prefetch_xyzi(rgbl_depth* h, const float* xyzi, int n, int w, int h_);
/* Forgets a prefetched scan that will not be followed by rgbl_depth_compute* (same reason as rgbl_extract_cancel: the scan is
 * recognised by pointer, n and ld).  Every other projecting entry point of the handle (the batch-device ones included)
 * invalidates a prefetch by itself. */
int rgbl_depth_prefetch_cancel(rgbl_depth* h);

/* The same on a scan as it lies in a KITTI velodyne .bin file: n records (x, y, z, reflectance).  Replaces
 * LoadPointcloudBinaryMat's repack to 4 x n (Examples/RGB-L/rgbl_kitti.cc:151-185: reflectance dropped, homogeneous
 * coordinate 1) plus CalculateDepthFromPcd; SURVEY.md 8(f) row f3. */
int rgbl_depth_compute_xyzi(rgbl_depth* h, const float* xyzi, int n, int w, int h_, const float* kp_xy,
                            const float* kpun_x, int k, float* out_depth, float* out_uright, float* out_raw,
                            float* out_processed);

/* Device-resident batch.  d_cloud: batch scans, scan b at d_cloud + b*cloud_stride floats, each 4 x n
 * with leading dimension ld.  Keypoints come straight from rgbl_extract_batch_device(): d_kp (frame b
 * at d_kp + b*kp_cap) and d_n (int32[batch]).  d_kpun_x may be NULL (undistorted == distorted, the
 * KITTI case, Frame.cc:837-845).  Outputs: d_depth/d_uright float[batch*kp_cap]; d_processed (nullable)
 * float[batch*h*w]. */
int rgbl_depth_batch_device(rgbl_depth* h, const float* d_cloud, int batch, int n, int ld,
                            size_t cloud_stride, int w, int h_, const rgbl_keypoint* d_kp,
                            const int32_t* d_n, int kp_cap, const float* d_kpun_x, float* d_depth,
                            float* d_uright, float* d_processed);
/* The two halves of the call above, for overlap: the projection / up-sampling half does not depend on the
 * keypoints, so it can run on the depth handle's stream while the extractor is still busy on its own. */
int rgbl_depth_project_batch_device(rgbl_depth* h, const float* d_cloud, int batch, int n, int ld,
                                    size_t cloud_stride, int w, int h_, float* d_processed);
/* projection half for scans in the .bin layout: scan b = n float4 records at d_xyzi + b*scan_stride floats
 * (16-byte aligned, scan_stride a multiple of 4) */
int rgbl_depth_project_xyzi_batch_device(rgbl_depth* h, const float* d_xyzi, int batch, int n, size_t scan_stride, int w,
                                         int h_, float* d_processed);
/* projection half for a batch of .bin scans of different lengths (KITTI scans hold ~115 k - 130 k points each), packed back
 * to back: scan b = records [d_offsets[b], d_offsets[b+1]) of d_xyzi (float4 x, y, z, reflectance; 16-byte aligned).
 * d_offsets: int64[batch + 1], device memory.  max_n >= every scan's count and <= cfg.max_points; it sizes the grid.  Point
 * indices stay local to their scan: "last point wins" (DepthModule.cc:123-137) holds per scan, every up-sampling method and
 * sparse handles work as with the fixed-n calls, an empty scan gives an empty depth map.  A scan longer than max_n is never
 * truncated silently: rgbl_depth_sync returns RGBL_ERR_OVERFLOW.  Enqueued on the handle's stream. */
int rgbl_depth_project_xyzi_varlen_batch_device(rgbl_depth* h, const float* d_xyzi, const int64_t* d_offsets, int batch,
                                                int max_n, int w, int h_, float* d_processed);
int rgbl_depth_gather_batch_device(rgbl_depth* h, int batch, int w, int h_, const rgbl_keypoint* d_kp,
                                   const int32_t* d_n, int kp_cap, const float* d_kpun_x, float* d_depth,
                                   float* d_uright);
int rgbl_depth_sync(rgbl_depth* h);
void* rgbl_depth_stream(rgbl_depth* h); /* hipStream_t currently used by the handle */
int rgbl_depth_set_stream(rgbl_depth* h, void* hip_stream);
/* Sparse up-sampling (off by default).  The reference fills ProcessedDepthMap for every frame (DepthModule.cc:203-251) and
 * then reads it at the keypoints only (DepthModule.cc:82-104); in RGB-L tracking nothing else reads it - its one consumer,
 * FrameDrawer.cc:375, is commented out.  With the switch on, an InverseDilation handle writes the dense map only for calls
 * that ask for it (out_processed / d_processed non-NULL); otherwise the keypoint gather evaluates the dilation at the
 * keypoints' pixels from the projected index map.  mvDepth / mvuRight are bit-identical either way. */
int rgbl_depth_set_sparse(rgbl_depth* h, int enable);
int rgbl_depth_profile(rgbl_depth* h, int enable);
int rgbl_depth_profile_read(rgbl_depth* h, const char** names, double* total_ms, long* launches, int cap);
int rgbl_depth_profile_samples(rgbl_depth* h, int kernel, float* ms, int cap);

/* ------------------------------------------------------------------------------------------------
 * ORBmatcher              replaces include/ORBmatcher.h:43,75-76, src/ORBmatcher.cc:907-1146,2058-2074
 * ---------------------------------------------------------------------------------------------- */
/* What a host-pointer matcher call costs (round 6): the handle owns a device arena and a page-locked block of the same layout;
 * everything a call uploads goes up with ONE request, its result arrays come back with one, the call synchronises once
 * (7 - 25 us beside its kernels).  A frame that is resident on the device (rgbl_device_frame, below) is not uploaded at all. */
typedef struct rgbl_matcher rgbl_matcher;
int rgbl_matcher_create(int device, rgbl_matcher** out);
void rgbl_matcher_destroy(rgbl_matcher* h);
/* Pooled handles for callers that build their matcher per call, as the reference does: `ORBmatcher matcher(0.9, true);`
 * is a function-local object in Tracking::TrackReferenceKeyFrame / TrackWithMotionModel / SearchLocalPoints / Relocalization
 * (Tracking.cc:2525, 2761, 2890, 3424, 3662, 3701) and LocalMapping::CreateNewMapPoints (LocalMapping.cc:412).  acquire gives
 * an idle handle of `device` (or creates the first ones), release parks it; the HIP stream and the device arena live on, so
 * constructing / destroying the drop-in class costs no HIP object.  Handles held at the same time are distinct. */
int rgbl_matcher_acquire(int device, rgbl_matcher** out);
void rgbl_matcher_release(rgbl_matcher* h);
int rgbl_matcher_pool_size(void);  /* idle handles (diagnostics / tests) */
int rgbl_matcher_pool_clear(void); /* destroys the idle handles (streams, device arenas, page-locked blocks): orderly shutdown; returns how many */
int rgbl_matcher_sync(rgbl_matcher* h);
int rgbl_matcher_set_stream(rgbl_matcher* h, void* hip_stream);
void* rgbl_matcher_stream(rgbl_matcher* h);
int rgbl_matcher_profile(rgbl_matcher* h, int enable);
int rgbl_matcher_profile_read(rgbl_matcher* h, const char** names, double* total_ms, long* launches, int cap);
int rgbl_matcher_profile_samples(rgbl_matcher* h, int kernel, float* ms, int cap);

/* static int ORBmatcher::DescriptorDistance(a, b) (ORBmatcher.cc:2058-2074) on two 32-byte rows. Host. */
int rgbl_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Hamming brute force: for every row of A the best and second-best row of B, selection rule of
 * ORBmatcher.cc:283-304 (strict '<': the first minimum wins; distances start at 256, idx at -1 - so a row at distance 256, a
 * complement, is never the best).  nb <= 65535: a train row's index travels in 16 bits (RGBL_ERR_INVALID beyond, nothing written).
 * Host pointers, synchronous.  second_dist may be NULL. */
int rgbl_hamming_bf(rgbl_matcher* h, const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb,
                    int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* Frame::ComputeStereoFishEyeMatches (/root/reference/src/Frame.cc:1256-1296) up to the triangulation:
 * the lapping-area subsets of both images - rows [mono_left, n_left) and [mono_right, n_right), monoLeft / monoRight being
 * what ORBextractor::operator() returned (Frame.cc:512-514) - matched by cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) and
 * Lowe's ratio test `size() >= 2 && best.distance < second.distance * 0.7`.  left_to_right[i] (n_left entries, indices into
 * the FULL right arrays like mvLeftToRightMatch) = the right keypoint that passed, else -1; best_dist / second_dist
 * (nullable, n_left entries, 256 = none) are the two knnMatch distances.  KannalaBrandt8::TriangulateMatches and the
 * `depth > 0.0001f` gate (Frame.cc:1287-1294) stay with the caller, who owns the camera objects.  Host pointers, synchronous. */
int rgbl_stereo_fisheye_matches(rgbl_matcher* h, const uint8_t* desc_left, int n_left, int mono_left, const uint8_t* desc_right,
                                int n_right, int mono_right, int32_t* left_to_right, int32_t* best_dist, int32_t* second_dist);
/* Device batch over frame pairs: descriptors of frame f live at d_desc + f*cap*32 with d_n[f] rows
 * (the layout rgbl_extract_batch_device() writes).  Pair p matches frame pair_a[p] (queries) against
 * frame pair_b[p] (train); outputs for pair p start at p*cap.  cap 1 .. 65535 (RGBL_ERR_INVALID beyond). */
int rgbl_hamming_bf_batch_device(rgbl_matcher* h, const uint8_t* d_desc, const int32_t* d_n, int cap,
                                 const int32_t* d_pair_a, const int32_t* d_pair_b, int n_pairs,
                                 int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_second_dist);

/* ---- Frames resident on the device ----------------------------------------------------------------------------------
 * A Frame / KeyFrame is matched many times (Tracking: SearchByProjection, SearchLocalPoints, SearchByBoW on the same
 * CurrentFrame; LocalMapping: SearchForTriangulation / Fuse of one key frame against ~10-20 neighbours), and its per-feature
 * arrays - mDescriptors, mvKeysUn[].pt / .octave, mvuRight (src/Frame.cc:110-125, 302-340; KeyFrame.cc:41-76) - never change
 * after construction.  An rgbl_device_frame holds them in HBM: filled ONCE, either from host arrays (one page-locked block,
 * one copy) or straight from the extractor / depth handles that produced them (device to device - the descriptors and
 * keypoints never cross PCIe a second time), and named by the `device` member of the views below, whose host pointers for
 * these four arrays are then not read.  Optionally the FeatureVector's CSR arrays as well.  A frame object is filled by one
 * thread at a time; once filled it may be read by any number of concurrent matcher calls. */
typedef struct rgbl_device_frame rgbl_device_frame;
int rgbl_device_frame_create(int device, int capacity /* features, 1 .. 65535: the matchers' 16-bit feature indices */, rgbl_device_frame** out);
void rgbl_device_frame_destroy(rgbl_device_frame* f);
/* n <= capacity features from host arrays; uright may be NULL (monocular: all -1).  Synchronous. */
int rgbl_device_frame_upload(rgbl_device_frame* f, int n, const uint8_t* desc, const float* kp_xy, const int32_t* kp_octave,
                             const float* uright);
/* The n keypoints / descriptors frame `frame` of the extractor's LAST rgbl_extract* call left on the device (n = the count
 * that call returned) and, with a depth handle, the mvuRight of ITS last rgbl_depth_compute* call (else -1).  K / dist
 * (nullable) = Frame::UndistortKeyPoints (Frame.cc:837-870): mvKeysUn from mvKeys; nothing is computed when dist is NULL or
 * dist[0] == 0, as upstream.  Enqueued on the extractor's stream behind that extraction; returns without waiting. */
int rgbl_device_frame_capture(rgbl_device_frame* f, rgbl_extractor* ex, int frame, int n, rgbl_depth* depth, const float K[4],
                              const float* dist, int n_dist);
/* mFeatVec as CSR (the node ids stay with the caller: the merge walk of two FeatureVectors is host work).  Call again after
 * upload / capture (they invalidate it).  Synchronous. */
int rgbl_device_frame_set_feature_vector(rgbl_device_frame* f, int n_nodes, const int32_t* node_off, const int32_t* node_feat);
/* Frame::AssignFeaturesToGrid (src/Frame.cc:475-506) for the frame's keypoints, kept with the frame: grid = Frame::mnMinX, mnMinY,
 * mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv.  A projection search whose input names this frame and the same six
 * values skips its grid build (11 - 15 us of a 75 - 90 us call).  Call after upload / capture (they invalidate it).  Synchronous. */
int rgbl_device_frame_set_grid(rgbl_device_frame* f, const float grid[6]);
int rgbl_device_frame_size(const rgbl_device_frame* f);
/* test / debug: the resident arrays back to the host (any pointer may be NULL) */
int rgbl_device_frame_download(rgbl_device_frame* f, uint8_t* desc, float* kp_xy, int32_t* kp_octave, float* uright);

/* int ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse)
 * (ORBmatcher.h:75-76, ORBmatcher.cc:907-1146) on flattened key-frames (mono / stereo pinhole,
 * mpCamera2 == nullptr).  The shim flattens KeyFrame under its mutexes, computes F12 and the epipole
 * once (Pinhole.cpp:109-112, ORBmatcher.cc:913-931) and rebuilds the pair vector from matches12. */
typedef struct {
  int n;                    /* KeyFrame::N */
  const uint8_t* desc;      /* mDescriptors, n x 32 */
  const float* kp_xy;       /* mvKeysUn[i].pt, n x 2 */
  const int32_t* kp_octave; /* mvKeysUn[i].octave */
  const float* kp_angle;    /* mvKeysUn[i].angle */
  const float* uright;      /* mvuRight */
  const uint8_t* has_mappoint; /* GetMapPoint(i) != NULL */
  /* mFeatVec (DBoW2::FeatureVector, a std::map<NodeId, vector<unsigned>>) as CSR, node ids ascending */
  int n_nodes;
  const int32_t* node_id;
  const int32_t* node_off;  /* n_nodes + 1 */
  const int32_t* node_feat; /* feature indices, ascending inside a node */
  /* nullable: the frame's resident copy - desc, kp_xy, kp_octave, uright above are then not read (and node_off / node_feat
   * only by the host-side passes, when the frame holds its FeatureVector: n_nodes must equal what was set) */
  const rgbl_device_frame* device;
} rgbl_keyframe_view;

typedef struct {
  float F12[9];                 /* K1^-T [t12]x R12 K2^-1, row-major */
  float epipole[2];             /* ep = project(T2w * Cw1) in image 2 */
  const float* scale_factors2;  /* pKF2->mvScaleFactors */
  const float* level_sigma2_2;  /* pKF2->mvLevelSigma2 */
  int n_levels;
  int only_stereo;              /* bOnlyStereo */
  int coarse;                   /* bCoarse */
  int check_orientation;        /* mbCheckOrientation (false for LocalMapping.cc:412's matcher) */
} rgbl_triangulation_params;

/* Host pointers, synchronous. matches12 has kf1->n entries (-1 = unmatched); *out_nmatches = return
 * value of the reference function. */
int rgbl_search_triangulation(rgbl_matcher* h, const rgbl_keyframe_view* kf1,
                              const rgbl_keyframe_view* kf2, const rgbl_triangulation_params* prm,
                              int32_t* matches12, int* out_nmatches);

/* void LocalMapping::CreateNewMapPoints() (include/LocalMapping.h, src/LocalMapping.cc:388-712) from its neighbour loop on
 * (:434-711), without the `new MapPoint` / AddObservation / Atlas part (:694-709), which stays with the caller.  Single-camera
 * pinhole key frames (mpCamera2 == nullptr, NLeft == -1; the rig branches :505-555 have no form here).
 * A key frame as the loop reads it: the view of rgbl_search_triangulation plus the per-match block's inputs (:481-691,
 * GeometricTools::Triangulate src/GeometricTools.cc:47-66, KeyFrame::UnprojectStereo src/KeyFrame.cc:755-772). */
typedef struct {
  rgbl_keyframe_view view;
  const float* depth;          /* mvDepth, n (host pointer also with a resident frame) */
  const float* kp_xy_raw;      /* mvKeys[i].pt, n x 2, what UnprojectStereo reads; NULL: the view's kp_xy (no distortion) */
  float Tcw[12];               /* GetPose().matrix3x4(), row-major; mRwc is taken as its rotation transposed */
  float Ow[3];                 /* GetCameraCenter() = mTwc.translation() */
  float K[4];                  /* fx, fy, cx, cy */
  float mb, mbf;
  const float* scale_factors;  /* mvScaleFactors, n_levels of the params */
  const float* level_sigma2;   /* mvLevelSigma2 */
} rgbl_new_points_keyframe;

typedef struct {
  int n_levels;
  float ratio_factor;          /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:428) */
  int far_points;              /* mbFarPoints */
  float th_far_points;         /* mThFarPoints */
  int inertial;                /* mbInertial: 0.9996 instead of 0.9998 (:583) */
  int monocular;               /* mbMonocular: no baseline test inside the call (:448-460), skip[] carries the median-depth one */
  int report_rejected;         /* 1: a record for every match, whatever its status; 0: accepted ones (status 1 - 3) only */
} rgbl_new_points_params;

/* status: 0 no match, 1 accepted triangulated, 2 / 3 accepted stereo point of key frame 1 / 2, 4 low parallax and no stereo
 * (:601-604), 5 w == 0, 6 UnprojectStereo false, 7 z1 <= 0, 8 z2 <= 0, 9 / 10 reprojection in key frame 1 / 2, 11 dist == 0,
 * 12 far point, 13 scale consistency.  x3D is zero for 4 - 6. */
typedef struct {
  int32_t neighbour, idx1, idx2;
  float x3D[3];
  uint8_t status;
  uint8_t reserved[3];         /* 0 */
} rgbl_new_point;

/* The per-match block (:481-691) on explicit pairs (idx1[i] of kf1, idx2[i] of kf2): one record per pair, in pair order,
 * neighbour = 0.  The views' FeatureVectors and descriptors are not read.  Host pointers, synchronous. */
int rgbl_triangulate_matches(rgbl_matcher* h, const rgbl_new_points_keyframe* kf1, const rgbl_new_points_keyframe* kf2,
                             const rgbl_new_points_params* prm, int n_pairs, const int32_t* idx1, const int32_t* idx2,
                             rgbl_new_point* out);
/* The loop :434-711 in one call: per neighbour kf2[i] the search (tri_prm[i]: F12, epipole, coarse, pKF2's tables;
 * only_stereo as given; check_orientation must be 0 as LocalMapping.cc:412 has it, else RGBL_ERR_INVALID - the rotation
 * histogram would be a host pass in the middle of the chain) and the per-match block, chained on the matcher's stream: an
 * accepted match gives kf1's feature a map point (:701) that the next neighbour's search skips.  One upload, one read-back.
 * skip (nullable): skip[i] != 0 leaves neighbour i out (the caller's monocular median-depth test, :455-459); with
 * monocular == 0 a neighbour with |Ow2 - Ow1| < kf2[i].mb is left out as well (:444-451).  matches_per_neighbour[i]
 * (nullable): -1 for a neighbour left out, else what SearchForTriangulation returned.
 * out: the records in the reference's order (neighbour, then ascending idx1), *n_out of them.  With report_rejected == 0 there
 * is at most one per feature of kf1 without a map point, so cap = kf1->view.n always suffices; more than cap records:
 * RGBL_ERR_CAPACITY with *n_out set, out and has_mappoint1_out untouched.  Every argument error is reported before anything
 * is launched and leaves all outputs untouched.  The read-back carries cap records whatever *n_out turns out to be (56 KB at
 * cap = 2000): a caller who knows a smaller bound shortens it.
 * has_mappoint1_out (nullable, n entries, may be kf1->view.has_mappoint itself): the mask after the call.
 * The `CheckNewKeyFrames()` poll between two neighbours (:436) has no device form: a caller who wants it splits the neighbours
 * over several calls and passes has_mappoint1_out on as the next call's kf1->view.has_mappoint.
 * Host pointers, synchronous. */
int rgbl_create_new_map_points(rgbl_matcher* h, const rgbl_new_points_keyframe* kf1, int n_neigh,
                               const rgbl_new_points_keyframe* kf2, const rgbl_triangulation_params* tri_prm,
                               const uint8_t* skip, const rgbl_new_points_params* prm, rgbl_new_point* out, int cap, int* n_out,
                               int32_t* matches_per_neighbour, uint8_t* has_mappoint1_out);
/* rgbl_triangulate_matches evaluated by the HOST build of csrc/newpoint_math.h (no device, no handle): what the tests compose
 * with the oracle's SearchForTriangulation into the restatement the device is compared with.  The views' resident frames are
 * not read: kp_xy, kp_octave and uright must be host arrays. */
int rgbl_triangulate_matches_host(const rgbl_new_points_keyframe* kf1, const rgbl_new_points_keyframe* kf2,
                                  const rgbl_new_points_params* prm, int n_pairs, const int32_t* idx1, const int32_t* idx2,
                                  rgbl_new_point* out);
/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) (include/ORBmatcher.h:57,
 * src/ORBmatcher.cc:223-425; callers Tracking::TrackReferenceKeyFrame, src/Tracking.cc:2798-2810, and Relocalization).
 * Single-camera frames.  kf: the key-frame (has_mappoint = GetMapPointMatches()[i] != NULL && !isBad(), kp_angle =
 * mvKeysUn[i].angle, FeatureVector as CSR); frame: F.mDescriptors, kp_angle = F.mvKeys[i].angle, F.mFeatVec (the other
 * fields of the view are not read).  match_f (frame->n entries): index of the key-frame feature whose map point ends up
 * in vpMapPointMatches[i], or -1.  Host pointers, synchronous.
 * All three SearchByBoW entry points: a vocabulary node the two sets share may hold at most 16384 features of the second set (the
 * frame; kf2) - a bucket position indexes one byte of LDS each; RGBL_ERR_INVALID beyond, before match_f / match12 is written. */
int rgbl_search_by_bow(rgbl_matcher* h, const rgbl_keyframe_view* kf, const rgbl_keyframe_view* frame, float nnratio,
                       int check_orientation, int32_t* match_f, int* out_nmatches);
/* The same for a two-camera frame (F.Nleft != -1: the fisheye rig; src/ORBmatcher.cc:298-326 and 357-386).  frame_n_left =
 * F.Nleft: the frame's features [0, frame_n_left) come from the left camera, the rest from the right one.  A key-frame feature
 * keeps a best / second best among the node's left features and a best among its right ones; if the left best is <= TH_LOW the
 * left one is taken under the ratio test and the right one whenever its own distance is <= TH_LOW (`|| true`, :359: no ratio
 * test) - so one key-frame feature can appear twice in match_f.  kp_angle of both views: the angle of the key point the
 * reference picks for that index (mvKeysUn / mvKeys / mvKeysRight, :335-343, :362-373).  frame_n_left = -1 is
 * rgbl_search_by_bow. */
int rgbl_search_by_bow_rig(rgbl_matcher* h, const rgbl_keyframe_view* kf, const rgbl_keyframe_view* frame, int frame_n_left,
                           float nnratio, int check_orientation, int32_t* match_f, int* out_nmatches);

/* int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (include/ORBmatcher.h:58,
 * src/ORBmatcher.cc:765-905; callers LoopClosing::DetectCommonRegionsFromBoW / DetectAndReffineSim3FromLastKF and
 * Tracking's relocalisation of the multi-map case).  Both views: has_mappoint = GetMapPointMatches()[i] != NULL && !isBad(),
 * kp_angle = mvKeysUn[i].angle, FeatureVector as CSR.  match12 (kf1->n entries): index of the kf2 feature whose map point ends
 * up in vpMatches12[i], or -1.  Host pointers, synchronous. */
int rgbl_search_by_bow_keyframes(rgbl_matcher* h, const rgbl_keyframe_view* kf1, const rgbl_keyframe_view* kf2, float nnratio,
                                 int check_orientation, int32_t* match12, int* out_nmatches);

/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono)
 * (include/ORBmatcher.h:48, src/ORBmatcher.cc:1676-1887; callers Tracking::TrackWithMotionModel, src/Tracking.cc:2917-2934):
 * the matcher that runs on every tracked frame.  Single-camera frames (Nleft == -1: RGB-L, RGB-D, stereo, mono pinhole).
 * Includes Frame::GetFeaturesInArea / AssignFeaturesToGrid / PosInGrid (src/Frame.cc:747-825, 475-506).  SURVEY.md 8(f) row f2.
 * CurrentFrame.mvpMapPoints is expected to be all NULL on entry, as Tracking.cc:2913 leaves it. */
typedef struct {
  int n1;                      /* LastFrame.N (< 2^20) */
  const uint8_t* valid1;       /* LastFrame.mvpMapPoints[i] != NULL && !LastFrame.mvbOutlier[i] */
  const float* world_pos1;     /* pMP->GetWorldPos(), 3 floats per feature */
  const uint8_t* mp_desc1;     /* pMP->GetDescriptor(), 32 bytes per feature */
  const uint8_t* mp_observed1; /* pMP->Observations() > 0: such a point blocks the feature it is assigned to (:1745-1747) */
  const int32_t* octave1;      /* LastFrame.mvKeys[i].octave */
  const float* angle1;         /* LastFrame.mvKeysUn[i].angle */
  int n2;                      /* CurrentFrame.N (<= 65535) */
  const float* kp2_xy;         /* CurrentFrame.mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* kp2_angle;
  const float* uright2;        /* CurrentFrame.mvuRight */
  const uint8_t* desc2;        /* CurrentFrame.mDescriptors */
  float grid[6];               /* Frame::mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  float Tcw_q[4], Tcw_t[3];    /* CurrentFrame.GetPose(): unit_quaternion() as (x, y, z, w), translation() */
  float Tlw_q[4], Tlw_t[3];    /* LastFrame.GetPose() */
  float K[4];                  /* fx, fy, cx, cy of CurrentFrame.mpCamera (Pinhole::project) */
  float mb, mbf;               /* CurrentFrame.mb, mbf */
  const float* scale_factors;  /* CurrentFrame.mvScaleFactors */
  int n_levels;
  float th;
  int mono;                    /* bMono */
  int check_orientation;       /* mbCheckOrientation */
  const rgbl_device_frame* device2; /* nullable: CurrentFrame resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
} rgbl_projection_input;
/* Host pointers, synchronous.  match2 has n2 entries: the index of the LastFrame feature whose map point the call leaves
 * in CurrentFrame.mvpMapPoints[i2], or -1.  *out_nmatches = return value of the reference function. */
int rgbl_search_by_projection(rgbl_matcher* h, const rgbl_projection_input* in, int32_t* match2, int* out_nmatches);

/* int ORBmatcher::SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th, const bool bFarPoints,
 * const float thFarPoints) (include/ORBmatcher.h:45, src/ORBmatcher.cc:43-213 with RadiusByViewingCos :215-221; caller
 * Tracking::SearchLocalPoints, src/Tracking.cc:3370-3450): the local map points that Frame::isInFrustum found visible are
 * searched around their predicted projection - best / second-best Hamming distance, ratio test inside one pyramid level.
 * Single-camera frames.  SURVEY.md 8(f) row f2. */
/* int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th,
 * const int ORBdist) (include/ORBmatcher.h:51, src/ORBmatcher.cc:1889-2010; caller Tracking::Relocalization,
 * src/Tracking.cc:3723-3752).  Single-camera frames.  The caller (shim) evaluates what needs the MapPoint objects:
 * valid1 and MapPoint::PredictScale (src/MapPoint.cc:531-546, a logf and a ceil); projection, window search, the greedy
 * assignment in key-frame index order and the rotation histogram are done here. */
typedef struct {
  int n1;                      /* pKF->GetMapPointMatches().size() (< 2^20) */
  const uint8_t* valid1;       /* pMP != NULL && !pMP->isBad() && !sAlreadyFound.count(pMP) &&
                                  minDistance <= |x3Dw - Ow| <= maxDistance (GetMin/MaxDistanceInvariance) */
  const float* world_pos1;     /* pMP->GetWorldPos(), 3 floats per point */
  const uint8_t* mp_desc1;     /* pMP->GetDescriptor(), 32 bytes per point */
  const int32_t* level1;       /* pMP->PredictScale(dist3D, &CurrentFrame) */
  const float* angle1;         /* pKF->mvKeysUn[i].angle */
  int n2;                      /* CurrentFrame.N (<= 65535) */
  const float* kp2_xy;         /* CurrentFrame.mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* kp2_angle;
  const uint8_t* desc2;        /* CurrentFrame.mDescriptors */
  const uint8_t* occupied2;    /* CurrentFrame.mvpMapPoints[i] != NULL on entry (nullable: none) */
  float grid[6];               /* Frame::mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  float Tcw_q[4], Tcw_t[3];    /* CurrentFrame.GetPose(): unit_quaternion() as (x, y, z, w), translation() */
  float K[4];                  /* fx, fy, cx, cy of CurrentFrame.mpCamera (Pinhole::project) */
  const float* scale_factors;  /* CurrentFrame.mvScaleFactors */
  int n_levels;
  float th;
  int orb_dist;                /* ORBdist, 0..255 */
  int check_orientation;       /* mbCheckOrientation */
  const rgbl_device_frame* device2; /* nullable: CurrentFrame resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
} rgbl_keyframe_projection_input;
/* Host pointers, synchronous.  match2 (n2 entries): index of the key-frame feature whose map point the call stores in
 * CurrentFrame.mvpMapPoints[i2], or -1 (entry left as it was).  *out_nmatches = return value of the reference function. */
int rgbl_search_by_projection_keyframe(rgbl_matcher* h, const rgbl_keyframe_projection_input* in, int32_t* match2,
                                       int* out_nmatches);

/* The per-point search of the Sim3-based loop-closing matchers: ORBmatcher::Fuse(KeyFrame* pKF, Sophus::Sim3f& Scw, const
 * vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint) (include/ORBmatcher.h:86, src/ORBmatcher.cc:1340-1455)
 * and both directions of SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (include/ORBmatcher.h:79, src/ORBmatcher.cc:1457-1674).
 * The caller (shim) applies its Sophus objects and evaluates the tests on the MapPoint objects; from the camera-frame
 * coordinates on - positive depth, projection, KeyFrame::IsInImage, the window of radius th * scale[level], octaves level - 1
 * ... level, the smallest Hamming distance - everything is done here, every point on its own. */
typedef struct {
  int n1;
  const uint8_t* valid1;       /* the point passed the caller's tests (NULL / bad / already matched / invariance range / viewing angle) */
  const float* cam_pos1;       /* the point in the key frame's camera frame (Tcw * p3Dw, resp. S21 * (T1w * p3Dw)), 3 floats */
  const uint8_t* mp_desc1;     /* pMP->GetDescriptor() */
  const int32_t* level1;       /* pMP->PredictScale(dist3D, pKF) */
  int n2;                      /* pKF->N (<= 65535) */
  const float* kp2_xy;         /* pKF->mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const uint8_t* desc2;
  float grid[6];               /* pKF->mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  float K[4];                  /* fx, fy, cx, cy */
  const float* scale_factors;
  int n_levels;
  float th;
  int proj_form;               /* 0: Pinhole::project (fx x / z + cx) as in Fuse; 1: invz = 1.0 / z (double), fx (x invz) + cx as in
                                  SearchBySim3; 2 (rgbl_search_by_projection_sim3 only): invz = 1 / z in float */
  int max_dist;                /* TH_LOW (Fuse) / TH_HIGH (SearchBySim3) */
  const rgbl_device_frame* device2; /* nullable: pKF resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
} rgbl_project_search_input;
/* Host pointers, synchronous.  best_idx[i] = key-frame feature with the smallest distance (<= max_dist) or -1; best_dist nullable. */
int rgbl_project_search(rgbl_matcher* h, const rgbl_project_search_input* in, int32_t* best_idx, int32_t* best_dist);

/* int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, int th, float ratioHamming) (include/ORBmatcher.h:61, src/ORBmatcher.cc:427-532; proj_form 0) and
 * the overload that also fills vpMatchedKF (include/ORBmatcher.h:65, src/ORBmatcher.cc:534-646; proj_form 2: invz = 1 / z in
 * float), the matchers of LoopClosing::FindMatchesByProjection.  Input as for rgbl_project_search (camera-frame points, the
 * caller's tests folded into valid1, max_dist = floor(TH_LOW * ratioHamming)); matched2[i] != 0: vpMatched[i] != NULL on entry
 * (nullable).  Points are taken in index order and a matched feature is skipped by the points after it.
 * match2 (n2 entries): index of the point stored in vpMatched[i2] by this call, or -1.  Host pointers, synchronous. */
int rgbl_search_by_projection_sim3(rgbl_matcher* h, const rgbl_project_search_input* in, const uint8_t* matched2, int32_t* match2,
                                   int* out_nmatches);

/* void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:329-403; called after every new observation / fusion, e.g.
 * LocalMapping.cc:333,691, Tracking.cc:2437) for a batch of map points: the N x N ORBmatcher::DescriptorDistance table of a point's
 * observed descriptors, and the row with the least median.  desc: the rows vDescriptors collects, point p = rows off[p] ..
 * off[p+1]) in the order the reference pushes them (off[0] = 0, at most 65535 per point).  best[p] = BestIdx inside the point's
 * own list (the descriptor to clone into mDescriptor), -1 for a point with no descriptor.  Host pointers, synchronous. */
int rgbl_distinctive_descriptors(rgbl_matcher* h, const uint8_t* desc, const int32_t* off, int n_points, int32_t* best);

/* The search inside int ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th, const bool bRight)
 * (include/ORBmatcher.h:83, src/ORBmatcher.cc:1148-1338, bRight = false; caller LocalMapping::SearchInNeighbors,
 * src/LocalMapping.cc:737-879, twice per neighbour key frame).  Every map point finds its best feature independently of
 * the others; what the loop then does with a match (MapPoint::Replace / AddObservation, KeyFrame::AddMapPoint) mutates the
 * caller's objects and stays in the shim, as do the tests that need the MapPoint object. */
typedef struct {
  int n1;                         /* vpMapPoints.size() */
  const uint8_t* valid1;          /* pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF) && minDistance <= dist3D <= maxDistance &&
                                     !(PO.dot(Pn) < 0.5 * dist3D) */
  const float* world_pos1;        /* pMP->GetWorldPos() */
  const uint8_t* mp_desc1;        /* pMP->GetDescriptor() */
  const int32_t* level1;          /* pMP->PredictScale(dist3D, pKF) */
  int n2;                         /* pKF->N (<= 65535) */
  const float* kp2_xy;            /* pKF->mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* uright2;           /* pKF->mvuRight */
  const uint8_t* desc2;           /* pKF->mDescriptors */
  float grid[6];                  /* pKF->mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  float Tcw_q[4], Tcw_t[3];       /* pKF->GetPose() */
  float K[4];                     /* fx, fy, cx, cy (pKF->mpCamera->project) */
  float bf;                       /* pKF->mbf */
  const float* scale_factors;     /* pKF->mvScaleFactors */
  const float* inv_level_sigma2;  /* pKF->mvInvLevelSigma2 */
  int n_levels;
  float th;
  const rgbl_device_frame* device2; /* nullable: pKF resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
} rgbl_fuse_input;
/* Host pointers, synchronous.  best_idx[i] = the key-frame feature point i would be fused with (bestDist <= TH_LOW), or -1;
 * best_dist (nullable) = bestDist, 256 when the point had no candidate. */
int rgbl_fuse_search(rgbl_matcher* h, const rgbl_fuse_input* in, int32_t* best_idx, int32_t* best_dist);

typedef struct {
  int n1;                      /* vpMapPoints.size() (< 2^20) */
  const uint8_t* valid1;       /* pMP->mbTrackInView && !(bFarPoints && pMP->mTrackDepth > thFarPoints) && !pMP->isBad() */
  const float* proj1;          /* pMP->mTrackProjX, mTrackProjY, mTrackProjXR: 3 floats per point */
  const int32_t* level1;       /* pMP->mnTrackScaleLevel */
  const float* view_cos1;      /* pMP->mTrackViewCos */
  const uint8_t* mp_desc1;     /* pMP->GetDescriptor(), 32 bytes per point */
  const uint8_t* mp_observed1; /* pMP->Observations() > 0 */
  int n2;                      /* F.N (<= 65535) */
  const float* kp2_xy;         /* F.mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* uright2;        /* F.mvuRight */
  const uint8_t* desc2;        /* F.mDescriptors */
  const uint8_t* blocked2;     /* F.mvpMapPoints[i] != NULL && ->Observations() > 0 on entry (nullable: none) */
  float grid[6];               /* Frame::mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  const float* scale_factors;  /* F.mvScaleFactors */
  int n_levels;
  float th;
  float nnratio;               /* mfNNratio */
  const rgbl_device_frame* device2; /* nullable: F resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
} rgbl_local_points_input;
/* Host pointers, synchronous.  match2 (n2 entries): index of the map point the call stores in F.mvpMapPoints[i2], or -1
 * (entry left as it was).  *out_nmatches = return value of the reference function. */
int rgbl_search_local_points(rgbl_matcher* h, const rgbl_local_points_input* in, int32_t* match2, int* out_nmatches);

/* ---- Tracking::SearchLocalPoints in one call: Frame::isInFrustum + MapPoint::PredictScale on the device -----------------
 * A pool of map-point data that lives on the device, the map-side counterpart of rgbl_device_frame: what Frame::isInFrustum
 * (src/Frame.cc:602-664) and the matcher read from a MapPoint - GetWorldPos(), GetNormal(), mfMinDistance, mfMaxDistance
 * (src/MapPoint.cc:500-512 return 0.8f / 1.2f times these; the RAW values are stored), GetDescriptor().  A slot is 64 bytes:
 * 12 + 12 + 4 + 4 + 32, kept as five arrays (SoA).  The caller owns the slot numbers (shim/LocalMap.h maps MapPoint* to slot).
 * Every call that touches a pool - update, reserve, a search that reads it - takes the pool's own mutex for its whole
 * duration, so LocalMapping may update while Tracking searches; calls on different pools are independent.  A slot that was
 * never updated reads as zeros. */
typedef struct rgbl_map_points rgbl_map_points;
int rgbl_map_points_create(int device, int capacity, rgbl_map_points** out);
void rgbl_map_points_destroy(rgbl_map_points* p);
/* grows the pool to at least `capacity` slots (never shrinks); the contents stay */
int rgbl_map_points_reserve(rgbl_map_points* p, int capacity);
int rgbl_map_points_capacity(rgbl_map_points* p);
/* Writes n slots: entry k of every non-NULL array goes to slot[k] (world_pos / normal 3 floats, desc 32 bytes per entry); a
 * NULL array leaves that field of the slots as it is.  A slot listed more than once takes its LAST entry.  RGBL_ERR_INVALID
 * for a slot outside [0, capacity) (nothing is written).  Host pointers, synchronous. */
int rgbl_map_points_update(rgbl_map_points* p, int n, const int32_t* slot, const float* world_pos, const float* normal,
                           const float* min_dist, const float* max_dist, const uint8_t* desc);

/* test / debug aid, like rgbl_device_frame_download: n slots back to the host, any array NULL */
int rgbl_map_points_download(rgbl_map_points* p, int n, const int32_t* slot, float* world_pos, float* normal,
                             float* min_dist, float* max_dist, uint8_t* desc);

/* ---- MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:426-494) and MapPoint::ComputeDistinctiveDescriptors (:329-403) on
 * the device: the pool's normal, mfMinDistance, mfMaxDistance and descriptor recomputed from observations given as
 * (key frame, feature) pairs of key frames that are resident on the device (rgbl_device_frame), for every listed point in
 * one call.  Single-camera key frames (rightIndex == -1); the caller leaves mbBad points out. */
typedef struct {
  int n_points;               /* <= 2^24 */
  const int32_t* slot;        /* pool slot of point p; each slot at most once per call (RGBL_ERR_INVALID otherwise) */
  const float* world_pos;     /* nullable: 3 floats per point, written to the slots FIRST (SetWorldPos after BA); NULL: the pool's */
  const int32_t* obs_off;     /* n_points + 1, from 0; point p's observations = [obs_off[p], obs_off[p+1]) in the order the reference
                                 iterates mObservations (std::map<KeyFrame*,...>: the caller's pointer order) */
  const int32_t* obs_kf;      /* index into the key-frame table below */
  const int32_t* obs_feat;    /* leftIndex of that observation */
  const int32_t* ref_kf;      /* per point: mpRefKF as an index into the table (read with do_normal) */
  const int32_t* ref_level;   /* per point: the octave the reference reads at :471-482 (incl. its quirk: observations[pRefKF]
                                 default-inserts (0,0) when the reference key frame does not observe the point -> feature 0) */
  int n_kfs;
  const rgbl_device_frame* const* kf_frame; /* resident key frames; an entry may be NULL only when do_descriptor == 0 */
  const float* kf_center;     /* GetCameraCenter(), 3 floats per key frame (read with do_normal) */
  const uint8_t* kf_bad;      /* pKF->isBad(): skipped by ComputeDistinctiveDescriptors (:352), NOT by UpdateNormalAndDepth; NULL: none */
  const float* scale_factors; /* pRefKF->mvScaleFactors (one table per call; a host with several extractor settings groups its calls) */
  int n_levels;               /* 1 .. 16 */
  int do_normal, do_descriptor;
} rgbl_map_refresh_input;
typedef struct {              /* every pointer nullable; n_points entries each */
  float* normal;              /* 3 per point */
  float* min_dist; float* max_dist;   /* RAW mfMinDistance / mfMaxDistance */
  int32_t* best_obs;          /* position inside the point's OWN observation list (bad key frames counted) of the descriptor that
                                 became mDescriptor, -1 = unchanged */
  uint8_t* desc;              /* 32 per point (the slot's descriptor after the call) */
  uint8_t* status;            /* bit 0: normal/distances written, bit 1: descriptor written */
} rgbl_map_refresh_output;
/* do_normal: a point without observations stays as it is (:441); otherwise normal = sum over ALL its observations, in list
 * order, of (Pos - Ow_kf) / |Pos - Ow_kf|, divided by their number; mfMaxDistance = |Pos - Ow_ref| * scale_factors[ref_level];
 * mfMinDistance = mfMaxDistance / scale_factors[n_levels - 1].  fp32 in the order of csrc/frustum_math.h, square root and
 * division correctly rounded; a point at a camera centre gives NaN as on the host.
 * do_descriptor: the rows are the observations of key frames that are not bad, in list order; none: the descriptor stays
 * (:365); otherwise the rule of rgbl_distinctive_descriptors picks the row whose 32 bytes go into the slot.
 * The result arrays hold the slots' values after the call, also for fields the call did not recompute.
 * RGBL_ERR_INVALID, before anything is launched or written: a slot outside the pool or listed twice; obs_kf / ref_kf outside
 * [0, n_kfs); obs_feat outside [0, rgbl_device_frame_size(frame)) (checked wherever the frame is given); ref_level outside
 * [0, n_levels) (ref_kf / ref_level are checked for every point, with do_normal); a NULL frame with do_descriptor; a frame or
 * pool on another device than the matcher; obs_off that does not start at 0 or descends; more than 65535 observations on
 * one point.  n_points == 0: RGBL_OK.
 * Holds the pool's mutex for its duration, runs on the handle's stream behind every key frame's last fill, one upload and one
 * read-back.  Host pointers, synchronous.  As for the matchers, a key frame must not be refilled (upload / capture) while the
 * call runs. */
int rgbl_map_points_refresh(rgbl_matcher* h, rgbl_map_points* pool, const rgbl_map_refresh_input* in, rgbl_map_refresh_output* out);

/* The frame side is that of rgbl_local_points_input; the map side is what the loop of Tracking::SearchLocalPoints
 * (src/Tracking.cc:3399-3420) reads before it calls isInFrustum, either as host arrays or as slots of a pool. */
typedef struct {
  int n1;                      /* mvpLocalMapPoints.size() (< 2^20) */
  const uint8_t* consider1;    /* pMP->mnLastFrameSeen != F.mnId && !pMP->isBad() (Tracking.cc:3406-3409); NULL: every point */
  /* map points, form 1 (pool == NULL): host arrays */
  const float* world_pos1;     /* pMP->GetWorldPos(), 3 floats per point */
  const float* normal1;        /* pMP->GetNormal(), 3 floats per point */
  const float* min_dist1;      /* pMP->mfMinDistance (GetMinDistanceInvariance() / 0.8f) */
  const float* max_dist1;      /* pMP->mfMaxDistance */
  const uint8_t* mp_desc1;     /* pMP->GetDescriptor(), 32 bytes per point (rgbl_frustum_cull does not read it) */
  /* map points, form 2: slots of a pool on the matcher's device; the five arrays above are then not read */
  rgbl_map_points* pool;
  const int32_t* slot1;        /* n1 slots in [0, capacity); any order, a slot may repeat */
  const uint8_t* mp_observed1; /* pMP->Observations() > 0 */
  int n2;                      /* F.N (<= 65535) */
  const float* kp2_xy;         /* F.mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* uright2;        /* F.mvuRight */
  const uint8_t* desc2;        /* F.mDescriptors */
  const uint8_t* blocked2;     /* F.mvpMapPoints[i] != NULL && ->Observations() > 0 on entry (nullable: none) */
  float grid[6];               /* Frame::mnMinX, mnMinY, mnMaxX, mnMaxY (also isInFrustum's image bounds), mfGridElementWidthInv, mfGridElementHeightInv */
  const float* scale_factors;  /* F.mvScaleFactors */
  int n_levels;                /* F.mnScaleLevels (1 .. 16) */
  float th;
  float nnratio;               /* mfNNratio */
  const rgbl_device_frame* device2; /* nullable: F resident on the device - kp2_xy, kp2_octave, uright2, desc2 are then not read */
  float Rcw[9], tcw[3], Ow[3]; /* F.mRcw (row-major), F.mtcw, F.mOw as Frame::UpdatePoseMatrices leaves them (Frame.cc:562-569) */
  float K[4];                  /* fx, fy, cx, cy of F.mpCamera (Pinhole::project, src/CameraModels/Pinhole.cpp:43-49) */
  float mbf;                   /* F.mbf */
  float log_scale_factor;      /* F.mfLogScaleFactor */
  float viewing_cos_limit;     /* isInFrustum's second argument: 0.5 (Tracking.cc:3411) */
  int far_points;              /* mpLocalMapper->mbFarPoints */
  float th_far_points;         /* mpLocalMapper->mThFarPoints */
} rgbl_track_local_input;
/* What isInFrustum leaves in a MapPoint (Frame.cc:605-607, 629-630, 653-661). */
typedef struct {
  float proj_x, proj_y;        /* mTrackProjX, mTrackProjY: (-1, -1) for a point rejected by depth or image bounds or not considered,
                                  the projection for one rejected by distance or viewing angle and for a point in view */
  float proj_xr, depth, view_cos; /* mTrackProjXR, mTrackDepth, mTrackViewCos of a point in view; 0 otherwise (the reference leaves them as they were) */
  int32_t level;               /* mnTrackScaleLevel = PredictScale(dist, &F) (src/MapPoint.cc:531-546) of a point in view; 0 otherwise */
} rgbl_frustum_record;
/* bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) (include/Frame.h:100, src/Frame.cc:602-664, the Nleft == -1
 * branch) for every considered point: in_view[i] = mbTrackInView (0 for a point that is not considered), rec (nullable) as
 * above, *n_in_view = the number of points in view = nToMatch (Tracking.cc:3399-3415).  The frame's feature arrays are not
 * read.  fp32 in the reference's order, logf as glibc 2.35 evaluates it (csrc/logf_glibc.h); a ratio mfMaxDistance / dist that
 * is not finite and positive, for which the reference's float -> int conversion is undefined, gives level 0.
 * Host pointers, synchronous.  Errors as for rgbl_search_local_points; a slot outside the pool: RGBL_ERR_INVALID. */
int rgbl_frustum_cull(rgbl_matcher* h, const rgbl_track_local_input* in, uint8_t* in_view, rgbl_frustum_record* rec, int* n_in_view);
/* Tracking.cc:3399-3448: the loop above and ORBmatcher::SearchByProjection(F, mvpLocalMapPoints, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:43-213) behind it, with one upload and one read-back.  in_view, rec (nullable), *n_to_match as for
 * rgbl_frustum_cull; match2 / *out_nmatches as for rgbl_search_local_points (all -1 / 0 when nothing is in view: the reference
 * does not call the matcher then, Tracking.cc:3422).  The search kernels are not launched when the host can tell that
 * nothing will be in view (no point considered, or n2 == 0); when the cull itself rejects every point they run over an
 * all-invalid list. */
int rgbl_track_local_points(rgbl_matcher* h, const rgbl_track_local_input* in, uint8_t* in_view, rgbl_frustum_record* rec,
                            int* n_to_match, int32_t* match2, int* out_nmatches);

/* int Optimizer::PoseOptimization(Frame* pFrame) (include/Optimizer.h, src/Optimizer.cc:814-1114): the motion-only bundle
 * adjustment Tracking runs after every search (src/Tracking.cc:2779, :2943, :3005 / :3011, :3748-3779), one workgroup per
 * frame.  Single-camera pinhole frames (pFrame->mpCamera2 == nullptr, Pinhole): monocular edges (uright < 0, :866-893) and
 * stereo / RGB-L edges (uright >= 0, :894-927) mixed; the rig branch (:930-991), KannalaBrandt8 and the inertial variants
 * (:4491, :4875) have no form here.  csrc/poseopt_math.h restates the function and the parts of g2o it runs, and says what is
 * pinned (control flow, the quirks, the summation order) and what is not (Eigen's LDLT, libm's sin / cos). */
typedef struct {
  int n;                       /* pFrame->N */
  const int32_t* mp_index;     /* per feature: index of pFrame->mvpMapPoints[i] in the map side below, -1 = no map point */
  int n_points;                /* entries of the map side */
  /* map side, form 1 (pool == NULL): host array */
  const float* world_pos;      /* pMP->GetWorldPos(), 3 floats per point */
  /* map side, form 2: slots of a pool on the matcher's device (the call holds the pool's mutex for its duration) */
  rgbl_map_points* pool;
  const int32_t* slot;         /* n_points slots in [0, capacity) */
  /* frame side: host arrays, or the resident frame (the three arrays are then not read) */
  const float* kp_xy;          /* mvKeysUn[i].pt, n x 2 */
  const int32_t* kp_octave;    /* mvKeysUn[i].octave */
  const float* uright;         /* mvuRight */
  const rgbl_device_frame* device;
  float Tcw_q[4];              /* GetPose().unit_quaternion(): x, y, z, w */
  float Tcw_t[3];              /* GetPose().translation() */
  float K[4];                  /* fx, fy, cx, cy (:916-919; the Pinhole's mvParameters for a monocular edge) */
  float bf;                    /* mbf */
  const float* inv_level_sigma2; /* mvInvLevelSigma2, n_levels entries */
  int n_levels;                /* 1 .. 16 */
} rgbl_pose_opt_input;
/* per round of :1006-1104 (rounds of them were run; the others are 0) */
typedef struct {
  int32_t iterations[4];       /* Levenberg iterations of the round's optimize() (0: no active edge) */
  int32_t active[4];           /* edges on level 0 when the round began */
  double chi2[4];              /* the robust chi2 of the active edges when optimize() returned (0 without iteration) */
  int32_t rounds, reserved;
  double Tcw_q[4], Tcw_t[3];   /* the vertex estimate in double, before :1109-1110 cast it to float */
} rgbl_pose_opt_diag;
typedef struct {
  float Tcw_q[4], Tcw_t[3];    /* what :1107-1111 hands to SetPose, x y z w; the input pose, bit for bit, when result is 0 because
                                  there are fewer than 3 correspondences (:996-997) */
  uint8_t* outlier;            /* mvbOutlier, n bytes, written only where mp_index >= 0 */
  int result;                  /* the reference's return value: nInitialCorrespondences - nBad */
  rgbl_pose_opt_diag diag;
} rgbl_pose_opt_output;
/* One frame (replaces Optimizer.cc:814-1114).  Host pointers, synchronous, one upload and one read-back.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: mp_index outside [-1, n_points); a slot
 * outside the pool; an octave outside [0, n_levels) on a feature with a map point (host arrays; a resident frame's octaves
 * are clamped on the device, the host does not hold them); a frame whose size is not n, or a frame or pool on another device
 * than the matcher; a pose, K or bf that is not finite; n_levels outside 1 .. 16; more than 65535 features. */
int rgbl_pose_optimization(rgbl_matcher* h, const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out);
/* B independent frames (the candidates of Tracking::Relocalization, :3748-3779, or an offline pipeline), each with its own
 * pose, K and bf, in ONE launch: the correspondences are packed back to back behind an offsets array, workgroup b runs
 * problem b.  One upload, one read-back.  A problem with n = 0 or fewer than 3 correspondences is valid (result 0).  Problems
 * that name a pool must name the same one.  Errors as above: nothing is launched and no problem's output is written. */
int rgbl_pose_optimization_batch(rgbl_matcher* h, int n_problems, const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out);
/* rgbl_pose_optimization evaluated by the HOST build of csrc/poseopt_math.h (no device, no handle): the same bits.  The
 * frame and map sides must be host arrays (device and pool NULL). */
int rgbl_pose_optimization_host(const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out);

/* Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc): the RANSAC over 3-point Horn solutions that
 * LoopClosing::DetectCommonRegionsFromBoW runs per candidate (src/LoopClosing.cc:698-710), ALL hypotheses of a call at once.
 * One call is what one or more calls of Sim3Solver::iterate (:149-294) compute: ComputeSim3 (:311-412) and CheckInliers
 * (:415-439) for every sample triple, then the rule by which the reference's loop stops (:192-209 / :265-287) as a scan over
 * the inlier counts.  Pinhole cameras (Pinhole::project, src/CameraModels/Pinhole.cpp:43-49).  csrc/sim3_math.h restates the
 * arithmetic and says what is pinned (fp32 / fp64 as the reference, SO3f::exp, the control flow) and what is not (the eigen
 * decomposition, atan2, Eigen's evaluation order).  The constructor's bookkeeping (:35-121), SetRansacParameters (:123-147)
 * and the drawing of the samples (:172-186) stay with the caller. */
typedef struct {
  int n;                       /* N = mvX3Dc1.size(), 0 .. 65535 */
  /* the points, form 1 (pool == NULL): camera frames, mvX3Dc1 / mvX3Dc2 (:107, :110), n x 3 */
  const float* x1c;
  const float* x2c;
  /* form 2: slots of a pool on the matcher's device and the two key-frame poses; the device forms Rcw * Xw + tcw in fp32 from
   * the resident positions (the call holds the pool's mutex for its duration) */
  rgbl_map_points* pool;
  const int32_t* slot1;        /* n slots in [0, capacity): pMP1 */
  const int32_t* slot2;        /* pMP2 */
  float Rcw1[9], tcw1[3];      /* pKF1->GetRotation() (row-major), GetTranslation() (:61-62); read in form 2 only */
  float Rcw2[9], tcw2[3];      /* pKF2's (:63-64) */
  const float* max_err1;       /* mvnMaxError1: 9.210 * sigma2 of the key point's level (:99) as the reference stores it - a
                                  std::vector<size_t>, so truncated to an integer -, n entries */
  const float* max_err2;       /* mvnMaxError2 (:100) */
  float K1[4], K2[4];          /* pCamera1 / pCamera2: fx, fy, cx, cy */
  int fix_scale;               /* mbFixScale */
  int min_inliers;             /* mRansacMinInliers */
  int best_inliers;            /* mnBestInliers on entry (0 for a fresh solver) */
  int n_hyp;                   /* iterations this call may run: min(nIterations, mRansacMaxIts - mnIterations); 0 .. 2^20 */
  const int32_t* samples;      /* n_hyp x 3 indices into 0 .. n-1 in the order drawn (:175-186), distinct inside a triple */
} rgbl_sim3_input;
typedef struct {
  int selected;                /* the hypothesis the loop holds when it ends (the last k with c[k] >= the best so far), -1: none */
  int converged;               /* 1: the scan stopped at a c[k] > min_inliers (:201 / :274) */
  int n_inliers;               /* c[selected]: the new mnBestInliers; 0 without a selection */
  int iterations_run;          /* k + 1 at the stop, n_hyp if the scan ran through: what mnIterations grows by */
  float T12[16];               /* mBestT12, row-major; with R12, t12, s12 and inlier written only when selected >= 0 */
  float R12[9];                /* mBestRotation, row-major */
  float t12[3];                /* mBestTranslation */
  float s12;                   /* mBestScale */
  uint8_t* inlier;             /* mvbBestInliers, n bytes (NULL: not wanted) */
  int32_t* counts;             /* optional diagnostics: mnInliersi of every hypothesis, n_hyp entries (NULL: not wanted) */
  float* T12_all;              /* optional diagnostics: mT12i of every hypothesis, n_hyp x 16 (NULL: not wanted) */
} rgbl_sim3_output;
/* One problem.  Host pointers, synchronous, one upload, two launches on one stream, one read-back.  A problem with n < 3,
 * n < min_inliers (:155-159) or n_hyp == 0 is valid: selected = -1 and nothing else is written.  Otherwise selected,
 * converged, n_inliers and iterations_run are always written, and so are counts and T12_all where given.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: n outside [0, 65535] or n_hyp outside
 * [0, 2^20] (SetRansacParameters' default mRansacMaxIts is 300); a sample index outside [0, n) or repeated in its triple
 * (n >= 3); K, a threshold or (form 2) a pose that is not finite; a slot outside the pool, or a pool on another device than
 * the matcher; a missing array. */
int rgbl_sim3_ransac(rgbl_matcher* h, const rgbl_sim3_input* in, rgbl_sim3_output* out);
/* B independent problems (the candidates of one DetectCommonRegionsFromBoW pass): one upload, one launch pair, one
 * read-back.  Problems that name a pool must name the same one.  Errors as above, and n_problems outside [0, 32767] (the
 * problem is a grid dimension): nothing is launched and no problem's output is written. */
int rgbl_sim3_ransac_batch(rgbl_matcher* h, int n_problems, const rgbl_sim3_input* in, rgbl_sim3_output* out);
/* rgbl_sim3_ransac evaluated by the HOST build of csrc/sim3_math.h (no device, no handle): the same bits.  The points must be
 * host arrays (pool NULL). */
int rgbl_sim3_ransac_host(const rgbl_sim3_input* in, rgbl_sim3_output* out);

/* MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp): the RANSAC over 6-point MLPnP solutions that
 * Tracking::Relocalization runs per candidate key frame (src/Tracking.cc:3690-3717), ALL hypotheses of a call at once, for
 * pinhole cameras without covariance information (covs(1), use_cov == false).  One call is what one call of
 * MLPnPsolver::iterate (:100-223) computes: computePose (:356-658) and CheckInliers (:262-293) for every sample, then the loop's
 * stop rule as a scan over the inlier counts.  Refine (:295-353) is what the reference COMPILES to: it never copies the pose it
 * computes into mRi / mti, so its CheckInliers sees the current hypothesis again; it succeeds iff that hypothesis has more than
 * min_inliers inliers, and iterate then returns that hypothesis (csrc/mlpnp_math.h, ml_scan).  The recomputed pose has no
 * observable effect and is not computed.  Batched, it covers the candidates of one pass of the
 * loop at Tracking.cc:3703.  csrc/mlpnp_math.h restates the arithmetic and says what is pinned and what is not.  The
 * constructor's bookkeeping (:55-97) is done here from the frame and the map side; SetRansacParameters (:225-260) and the
 * drawing of the samples (:128-140) stay with the caller.  N below = the number of features with mp_index >= 0: the
 * correspondences, in ascending feature index. */
typedef struct {
  int n;                       /* vpMapPointMatches.size() = F.N, 0 .. 65535 */
  const int32_t* mp_index;     /* per feature: index of vpMapPointMatches[i] in the map side below, -1 = none (or isBad) */
  int n_points;                /* entries of the map side */
  /* map side, form 1 (pool == NULL): host array */
  const float* world_pos;      /* pMP->GetWorldPos(), 3 floats per point (:84-86) */
  /* map side, form 2: slots of a pool on the matcher's device (the call holds the pool's mutex for its duration) */
  rgbl_map_points* pool;
  const int32_t* slot;         /* n_points slots in [0, capacity) */
  /* frame side: host arrays, or the resident frame (the two arrays are then not read) */
  const float* kp_xy;          /* F.mvKeysUn[i].pt, n x 2 (:72-74) */
  const int32_t* kp_octave;    /* F.mvKeysUn[i].octave (:75) */
  const rgbl_device_frame* device;
  float K[4];                  /* the Pinhole's fx, fy, cx, cy */
  const float* level_sigma2;   /* F.mvLevelSigma2, n_levels entries */
  int n_levels;                /* 1 .. 16 */
  float th2;                   /* SetRansacParameters' th2: mvMaxError[i] = sigma2 * th2 (:259) */
  int min_inliers;             /* mRansacMinInliers AFTER SetRansacParameters (:237-242), >= 6 */
  int best_inliers;            /* mnBestInliers on entry (0 for a fresh solver) */
  const uint8_t* best_mask;    /* mvbBestInliers on entry, N bytes; not read when best_inliers == 0 */
  float best_Tcw[16];          /* mBestTcw on entry, row-major */
  int n_hyp;                   /* iterations this call runs unless it succeeds earlier: max(mRansacMaxIts - mnIterations,
                                  nIterations) (the `||` of :115); 0 .. 2^20 */
  const int32_t* samples;      /* n_hyp x 6 indices into the correspondences 0 .. N-1 in the order drawn, distinct in a set */
} rgbl_mlpnp_input;
typedef struct {
  int found;                   /* iterate's return value */
  int no_more;                 /* bNoMore: 1 when the call ran through all n_hyp, or N < min_inliers */
  int n_inliers;               /* nInliers (0 when not found) */
  int iterations_run;          /* what mnIterations grows by: k + 1 at a successful Refine, else n_hyp */
  float Tcw[16];               /* Tout, row-major: hypothesis k's pose in float after a successful Refine (mRefinedTcw as compiled),
                                  mBestTcw after a run-through, identity when not found */
  uint8_t* inlier;             /* vbInliers, n bytes per FEATURE (through mvKeyPointIndices); written when found (NULL: not wanted) */
  int best_inliers;            /* the new mnBestInliers */
  uint8_t* best_mask;          /* the new mvbBestInliers, N bytes; written when the new best_inliers > 0 (NULL: not wanted) */
  float best_Tcw[16];          /* the new mBestTcw */
  int refines;                 /* diagnostics: how often the reference would have called Refine (the qualifying hypotheses up to the stop) */
  int32_t* counts;             /* optional diagnostics: mnInliersi of every hypothesis, n_hyp entries (NULL: not wanted) */
  double* Tcw_all;             /* optional diagnostics: [R | t] of every hypothesis in fp64, n_hyp x 12 row-major (NULL: not wanted) */
  int32_t* gn_path;            /* TEST DIAGNOSTICS, not a stable part of the interface - the encoding may change with the header: per
                                  hypothesis the Gauss-Newton updates + 8 (left at the break rule), + 16 (the stop rule), + 32 (a failed
                                  solve or non-finite step), n_hyp entries (NULL: not wanted).  The tests need it to tell which
                                  hypotheses took the model's path */
} rgbl_mlpnp_output;
/* One problem.  Host pointers, synchronous, one upload, two launches on one stream, one read-back.  Valid inputs that compute
 * nothing, as :106-110 does: N < min_inliers gives no_more = 1, found = 0; n_hyp == 0 gives found = 0, no_more = 0; in both the
 * state goes from the input to the output unchanged, Tcw is the identity, counts / Tcw_all / gn_path are not written.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: n outside [0, 65535]; n_hyp outside
 * [0, 2^20]; a sample outside [0, N) or repeated in its set; N < 6 with n_hyp > 0 and N >= min_inliers; min_inliers < 6;
 * mp_index outside [-1, n_points); a slot outside the pool; a pool or frame on another device than the matcher, or a frame
 * whose size is not n; an octave outside [0, n_levels) on a feature with a map point (host arrays; a resident frame's octaves
 * are clamped on the device); n_levels outside 1 .. 16; a K, th2 or sigma2 that is not finite; best_inliers < 0, or > 0 with a
 * best_mask that is missing or does not hold exactly best_inliers (>= 6) ones; a missing array; more than 2^26 mask words in
 * the call, i.e. the sum over the problems of n_hyp x ceil(N / 64) (512 MB of device scratch: 2^20 hypotheses of up to 4096
 * correspondences, or 65535 correspondences with up to 65536 hypotheses - each maximum alone is inside, both at once are not).
 * Beyond the checks a call can fail with RGBL_ERR_HIP when the device cannot hold its arena; nothing is written then either. */
int rgbl_mlpnp_ransac(rgbl_matcher* h, const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out);
/* B independent problems (the candidates of one pass of the loop at Tracking.cc:3703): one upload, one launch pair, one
 * read-back.  Problems that name a pool must name the same one.  Errors as above, and n_problems outside [0, 32767] (the
 * problem is a grid dimension): nothing is launched and no problem's output is written. */
int rgbl_mlpnp_ransac_batch(rgbl_matcher* h, int n_problems, const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out);
/* rgbl_mlpnp_ransac evaluated by the HOST build of csrc/mlpnp_math.h (no device, no handle): the same bits.  Frame and map
 * side must be host arrays (device and pool NULL). */
int rgbl_mlpnp_ransac_host(const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out);

/* bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated) (include/TwoViewReconstruction.h,
 * src/TwoViewReconstruction.cc:41-129), the step of Tracking::MonocularInitialization (src/Tracking.cc:2538) behind
 * SearchForInitialization, reached through Pinhole::ReconstructWithTwoViews (src/CameraModels/Pinhole.cpp:83-92): ALL
 * homography and fundamental hypotheses of a call at once.  One call replaces FindHomography and FindFundamental (:131-230) with
 * Normalize, ComputeH21, ComputeF21, CheckHomography and CheckFundamental (:232-473, :737-784), the choice of :112-128, and
 * ReconstructF / ReconstructH with DecomposeE and CheckRT (:475-734, :786-927).  csrc/twoview_math.h restates the arithmetic
 * and says what is pinned (the plain C++: precisions, orders, the serial score sums, every rule and quirk) and what is not
 * (what Eigen computes).  The drawing of the sets (:78-98) stays with the caller.  N below = the number of keys of frame 1 with
 * matches12 >= 0: the matches, in ascending index of frame 1 (mvMatches12). */
typedef struct {
  int n1, n2;                   /* vKeys1.size(), vKeys2.size(), 0 .. 65535 each */
  /* the keys: host arrays, or resident frames (the arrays are then not read) */
  const float* kp1_xy;          /* vKeys1[i].pt (mvKeysUn), n1 x 2 */
  const float* kp2_xy;          /* vKeys2[i].pt, n2 x 2 */
  const rgbl_device_frame* device1;
  const rgbl_device_frame* device2;
  const int32_t* matches12;     /* n1 entries: index into frame 2, -1 = none; what rgbl_search_initialization returns */
  float K[4];                   /* mK: fx, fy, cx, cy */
  float sigma;                  /* mSigma (1.0 at Pinhole.cpp:87) */
  int n_hyp;                    /* mMaxIterations (200 there), 0 .. 2^20 */
  const int32_t* samples;       /* mvSets: n_hyp x 8 indices into the matches 0 .. N-1, distinct in a set, drawn as :83-98 draws them */
} rgbl_two_view_input;
typedef struct {
  int found;                    /* Reconstruct's return value */
  int model;                    /* 0 = ReconstructH ran, 1 = ReconstructF ran, -1 = the SH + SF == 0 exit (:113) */
  int exit_code;                /* 0 found; 1 SH + SF == 0 (:113); 2 ReconstructH's d1 / d2, d2 / d3 exit (:597-600); 3 its final
                                   rule (:725-733); 4 ReconstructF's maxGood < nMinGood || nsimilar > 1 (:520-523); 5 its
                                   winner lacks parallax (:568) */
  float SH, SF;                 /* the two scores */
  int best_h, best_f;           /* the hypotheses that hold them; -1: no score > 0, H21 / F21 stay unset in the reference (zeros here) */
  float H21[9], F21[9];         /* row-major */
  float R21[9], t21[3];         /* T21 as the R and t handed to Sophus::SE3f (:533 .. :563, :727); identity and zeros when not found */
  float* p3d;                   /* n1 x 3: the WINNING motion hypothesis's vP3D, by the index of frame 1 - also on the homography
                                   path; written when found (NULL: not wanted) */
  uint8_t* triangulated;        /* vbTriangulated, n1 bytes; written when found (NULL: not wanted) */
  int p3d_assigned;             /* 1 where the reference assigns vP3D (the fundamental path), 0 where it leaves the caller's vector
                                   alone: ReconstructH drops bestP3D (:725-731) */
  int n_inliers;                /* N of ReconstructF / ReconstructH: the ones of the chosen mask (0 for model -1) */
  int best_motion;              /* the motion hypothesis the rule looked at: 0 .. 3 (F: R1 t, R2 t, R1 -t, R2 -t), 0 .. 7 (H), -1 none */
  int aux;                      /* nsimilar (F) or secondBestGood (H) */
  int n_good[8];                /* CheckRT's return value per motion hypothesis (F: the first four), zeros where none ran */
  float parallax[8];            /* CheckRT's parallax per motion hypothesis, degrees */
  float* scores;                /* optional diagnostics: currentScore of every hypothesis, n_hyp x 2 (H, F) (NULL: not wanted) */
  float* models;                /* optional diagnostics: H21i / F21i of every hypothesis, n_hyp x 2 x 9 */
  uint8_t* inliers_h;           /* optional diagnostics: vbMatchesInliersH, N bytes per MATCH */
  uint8_t* inliers_f;           /* optional diagnostics: vbMatchesInliersF, N bytes; NOT written when best_f == -1: that mask is
                                   EMPTY in the reference (FindFundamental sizes it by the empty argument, :185) */
} rgbl_two_view_output;
/* One problem.  Host pointers, synchronous, one upload, five launches on one stream, one read-back.  n_hyp == 0 is valid and
 * launches nothing: both scores stay 0, so model = -1, exit_code = 1, found = 0 (scores / models / masks are not written).
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: n1 or n2 outside [0, 65535]; n_hyp outside
 * [0, 2^20]; N < 8 with n_hyp > 0 (the reference would index an empty vector; Tracking never calls below 100 matches); a
 * sample outside [0, N) or repeated in its set; a match outside [-1, n2); a K or sigma that is not finite; a frame on another
 * device than the matcher or whose size is not n1 / n2; a missing array; more than 2^26 mask words in the call, i.e. the sum
 * over the problems of 2 x n_hyp x ceil(N / 64) (512 MB of device scratch); more than 2^24 keys of frame 1 in the call, summed over the
 * problems with n_hyp > 0 (CheckRT keeps 8 x 13 bytes per key: 1.7 GB).  Beyond the checks a call can fail with
 * RGBL_ERR_HIP when the device cannot hold its arena; nothing is written then either. */
int rgbl_two_view_reconstruct(rgbl_matcher* h, const rgbl_two_view_input* in, rgbl_two_view_output* out);
/* B independent problems: one upload, one launch sequence, one read-back.  Errors as above, and n_problems outside
 * [0, 32767] (the problem is a grid dimension): nothing is launched and no problem's output is written. */
int rgbl_two_view_reconstruct_batch(rgbl_matcher* h, int n_problems, const rgbl_two_view_input* in, rgbl_two_view_output* out);
/* rgbl_two_view_reconstruct evaluated by the HOST build of csrc/twoview_math.h (no device, no handle): the same bits.  The
 * keys must be host arrays (device1 and device2 NULL). */
int rgbl_two_view_reconstruct_host(const rgbl_two_view_input* in, rgbl_two_view_output* out);

/* int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
 * const bool bFixScale, Eigen::Matrix<double,7,7>& mAcumHessian, const bool bAllPoints) (include/Optimizer.h,
 * src/Optimizer.cc:2115-2381): the 7-dof refinement LoopClosing runs per candidate (src/LoopClosing.cc:556, :767), one
 * workgroup per candidate.  Pinhole cameras.  csrc/sim3opt_math.h restates the function and the parts of g2o it runs - the
 * numeric Jacobians of base_binary_edge.hpp included - and says what is pinned (control flow, the quirks, the summation
 * order) and what is not (Eigen's LDLT, libm's exp / sin / cos).  mAcumHessian is zeros on return (:2356): the caller
 * writes them. */
typedef struct {
  int n;                       /* vpMatches1.size() == pKF1->N */
  const int32_t* mp1_index;    /* per feature of pKF1: pKF1->GetMapPointMatches()[i] in the point set below, -1 = null */
  const int32_t* match_index;  /* vpMatches1[i] in the point set, -1 = null */
  const int32_t* i2;           /* get<0>(vpMatches1[i]->GetIndexInKeyFrame(pKF2)), -1 .. n2-1; read where match_index >= 0 */
  const int32_t* track_level2; /* the level of the inverse edge where i2 < 0, in [0, n_levels2).  :2280 names mnTrackScaleLevel, but hands it to
                                  cv::KeyPoint as the SIZE: as compiled with OpenCV the octave is 0, which is what
                                  shim/Sim3Optimizer.h passes and tests/golden/sim3_opt records */
  int n_points;                /* entries of the point set */
  const uint8_t* bad;          /* isBad() of every point */
  /* map side, form 1 (pool == NULL): host array */
  const float* world_pos;      /* GetWorldPos(), 3 floats per point */
  /* map side, form 2: slots of a pool on the matcher's device (the call holds the pool's mutex for its duration) */
  rgbl_map_points* pool;
  const int32_t* slot;         /* n_points slots in [0, capacity) */
  float Rcw1[9], tcw1[3];      /* pKF1->GetRotation() (row-major), GetTranslation() (:2129-2130) */
  float Rcw2[9], tcw2[3];      /* pKF2's (:2131-2132) */
  /* key frame 1: host arrays, or the resident frame (the two arrays are then not read) */
  const float* kp1_xy;         /* pKF1->mvKeysUn[i].pt, n x 2 */
  const int32_t* kp1_octave;
  const rgbl_device_frame* device1;
  int n2;                      /* pKF2->N */
  const float* kp2_xy;         /* pKF2->mvKeysUn, n2 x 2 */
  const int32_t* kp2_octave;
  const rgbl_device_frame* device2;
  const float* inv_level_sigma2_1; /* pKF1->mvInvLevelSigma2, n_levels1 entries */
  int n_levels1;               /* 1 .. 16 */
  const float* inv_level_sigma2_2;
  int n_levels2;
  float K1[4], K2[4];          /* pCamera1 / pCamera2: fx, fy, cx, cy */
  double q[4], t[3], s;        /* g2oS12 as g2o::Sim3 holds it: r (x y z w), t, s; never normalised */
  float th2;
  int fix_scale;               /* bFixScale */
  int all_points;              /* bAllPoints */
} rgbl_sim3_opt_input;
typedef struct {
  int32_t n_correspondences, n_bad_mps, n_in_kf2, n_out_kf2, n_without_mp; /* the counters of :2159-2163 */
  int32_t n_bad;               /* pairs dropped after the first optimize() (:2311) */
  int32_t iterations[2];       /* Levenberg iterations of the two optimize() calls (0: no edge, or not run) */
  int32_t active[2];           /* edge pairs in the graph when each began */
  double chi2[2];              /* the (robust) chi2 when each returned */
  int32_t rounds, reserved;    /* optimize() calls reached: 1 when the function returns at :2349 */
} rgbl_sim3_opt_diag;
typedef struct {
  int result;                  /* the reference's return value: nIn, or 0 */
  double q[4], t[3], s;        /* g2oS12 on return: the input estimate, bit for bit, when the function returns at :2349 */
  uint8_t* cleared;            /* n bytes (NULL: not wanted): 1 where the reference sets vpMatches1[idx] = NULL (:2323, :2369), 0
                                  where the pair stays; written only where an edge pair existed */
  rgbl_sim3_opt_diag diag;
} rgbl_sim3_opt_output;
/* One candidate (replaces Optimizer.cc:2115-2381).  Host pointers, synchronous, one upload, one launch, one read-back.  A
 * problem with no edge pair at all is valid: result 0 and no iteration.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: mp1_index / match_index outside
 * [-1, n_points); i2 outside [-1, n2); an octave (host arrays; a resident frame's octaves are clamped on the device) or
 * track_level2 outside [0, n_levels) on a pair that reaches the depth test of :2235; a pose, K, th2 or estimate that is not
 * finite; n or n2 above 65535; n_levels outside 1 .. 16; a slot outside the pool; a frame of another size, or a frame or pool
 * on another device than the matcher; a missing array. */
int rgbl_optimize_sim3(rgbl_matcher* h, const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out);
/* B independent candidates (one DetectCommonRegionsFromBoW pass, LoopClosing.cc:690-800): one upload, one launch, one
 * read-back; workgroup b runs problem b.  Problems that name a pool must name the same one.  Errors as above, and n_problems
 * outside [0, 32767]: nothing is launched and no problem's output is written. */
int rgbl_optimize_sim3_batch(rgbl_matcher* h, int n_problems, const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out);
/* rgbl_optimize_sim3 evaluated by the HOST build of csrc/sim3opt_math.h (no device, no handle): the same bits.  Both key
 * frames and the map side must be host arrays (device1, device2 and pool NULL). */
int rgbl_optimize_sim3_host(const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out);

/* Optimizer::LocalBundleAdjustment(KeyFrame*, bool* pbStopFlag, Map*, ...)    src/Optimizer.cc:1116-1498, from :1188 on: the
 * one optimize(10) of LocalMapping's bundle adjustment, ONE problem spread over the device - linearisation per edge, the Schur
 * complement one workgroup per block of the reduced camera system, its LDL^T, back-substitution per point -, with Levenberg's
 * scalar control on the host between launches, where the stop flag is polled exactly where g2o polls it.  Single-camera
 * pinhole key frames, monocular and stereo / RGB-L edges mixed.  csrc/lba_math.h restates the arithmetic and says what is
 * pinned (every summation order, g2o's Levenberg with its quirks) and what is not (SimplicialLDLT's elimination order,
 * Eigen's evaluation order).  The graph walk (:1118-1186), the edge loop (:1282-1403) and the write-back (:1413-1497) stay
 * with the caller. */
typedef struct {
  int n_free;                      /* lLocalKeyFrames, in list order; 0 .. 128 */
  int n_fixed;                     /* lFixedCameras; 0 .. 1024 */
  const uint8_t* free_is_fixed;    /* n_free bytes (NULL: none): 1 for the map's initial key frame (:1220) */
  const float* cam_q;              /* (n_free + n_fixed) x 4, free cameras first: GetPose().unit_quaternion() as x, y, z, w */
  const float* cam_t;              /* (n_free + n_fixed) x 3: GetPose().translation() */
  const float* cam_K;              /* (n_free + n_fixed) x 4: fx, fy, cx, cy */
  const float* cam_bf;             /* n_free + n_fixed: mbf */
  int n_points;                    /* lLocalMapPoints, in list order; 0 .. 2^18 */
  const float* world_pos;          /* form 1 (pool == NULL): n_points x 3 */
  rgbl_map_points* pool;           /* form 2: slots of a pool on the matcher's device, each at most once (the call holds the */
  const int32_t* slot;             /*   pool's mutex for its duration) */
  int n_edges;                     /* 0 .. 2^20, in the order the reference creates them */
  const int32_t* edge_point;       /* non-decreasing */
  const int32_t* edge_cam;         /* an index into free ++ fixed; a (point, camera) pair at most once */
  const float* edge_obs;           /* n_edges x 3: kpUn.pt.x, kpUn.pt.y, mvuRight (< 0: a monocular edge) */
  const float* edge_inv_sigma2;    /* mvInvLevelSigma2[kpUn.octave] */
  int max_iterations;              /* optimize(10) */
  double user_lambda_init;         /* > 0 replaces computeLambdaInit (:1197-1198: 100 for an inertial map) */
  const volatile int32_t* stop;    /* pbStopFlag (NULL: none), read where g2o's terminate() reads it */
  int stop_after_polls;            /* for tests: N > 0 makes the flag read as set from the N-th poll on (poll 1 is :1406) */
  const volatile uint8_t* stop_byte; /* the same flag as a one-byte C++ bool (NULL: none), read at the same polls: set when either is */
} rgbl_lba_input;
typedef struct {
  int32_t ran;                     /* 0: returned at :1182-1186 (no fixed camera) or :1406-1408 (stop set); nothing else is written */
  int32_t iterations, trials;      /* solve() calls, and the Levenberg trials of all of them */
  int32_t rejected, failed;        /* trials that were popped, and trials whose factorisation failed */
  int32_t active_cams, active_points;
  int32_t polls;                   /* how often the stop flag was read */
  double first_chi2, last_chi2;    /* activeRobustChi2 before the first step and Levenberg's currentChi at the end */
  double last_lambda;
  double* cam_q;                   /* optional (NULL: not wanted): the vertex estimates in double, n_free x 4 ... */
  double* cam_t;                   /* ... n_free x 3 ... */
  double* point;                   /* ... and n_points x 3 */
} rgbl_lba_diag;
typedef struct {
  float* cam_q;                    /* n_free x 4: what :1483-1485 hands to SetPose, x y z w (the estimate cast to float) */
  float* cam_t;                    /* n_free x 3 */
  float* point;                    /* n_points x 3: what :1493 hands to SetWorldPos */
  double* chi2;                    /* n_edges: e->chi2() as :1425 / :1455 read it (the last TRIED step; 0 if never computed) */
  uint8_t* flags;                  /* n_edges: bit 0 = erase (:1425 / :1455), bit 1 = the depth is not positive */
  rgbl_lba_diag diag;
} rgbl_lba_output;
/* Host pointers, synchronous; every launch goes on the matcher's stream.  A camera or point without an edge is not active and
 * comes back as the float -> double -> float round trip of its input; a call without any edge runs no iteration.  No fixed
 * camera at all (n_fixed == 0 and no free_is_fixed) and a stop flag that is set on entry are valid: diag.ran = 0 and no array,
 * nor the pool, is written.  With a pool the optimised positions are also written into the slots, only when ran = 1.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: a count outside its range above;
 * edge_point / edge_cam out of range; edge_point decreasing; a repeated (point, camera) pair; a pose, K or bf that is not
 * finite; a slot outside the pool or listed twice; a pool on another device than the matcher; a missing array. */
int rgbl_local_bundle_adjustment(rgbl_matcher* h, const rgbl_lba_input* in, rgbl_lba_output* out);
/* The same call evaluated by the HOST build of csrc/lba_math.h (no device, no handle): the same bits.  pool must be NULL. */
int rgbl_local_bundle_adjustment_host(const rgbl_lba_input* in, rgbl_lba_output* out);

/* Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)    src/Optimizer.cc:52-390, the
 * optimize(nIterations) at :281: the global bundle adjustment behind Optimizer::GlobalBundleAdjustemnt - LoopClosing.cc:2284
 * (10 iterations, mbStopGBA, not robust) and Tracking.cc:2614 (20 iterations) -, as ONE problem spread over the device.  The
 * edges, the block solver with the Schur complement and Levenberg are rgbl_local_bundle_adjustment's (csrc/lba_math.h) and so
 * are their kernels; the reduced camera system, up to 6 144 unknowns, is factorised and solved in panels of columns across the
 * device (csrc/gba.hip, lm_solve_panel of csrc/lm_math.h: lm_solve_n's L, D and y, the backward substitution in the mirrored
 * order).  The vertex and edge loops (:116-275) and the write-back (:285-389) stay with the caller. */
typedef struct {
  int n_cams;                      /* vpKFs without the bad ones, in list order; 0 .. 2048 */
  const uint8_t* cam_is_fixed;     /* n_cams bytes (NULL: none): 1 for the map's initial key frame (:125); at most 1024 set */
  const float* cam_q;              /* n_cams x 4: GetPose().unit_quaternion() as x, y, z, w */
  const float* cam_t;              /* n_cams x 3 */
  const float* cam_K;              /* n_cams x 4: fx, fy, cx, cy */
  const float* cam_bf;             /* n_cams: mbf */
  int n_points;                    /* vpMP without the bad ones, in list order; 0 .. 2^18 */
  const float* world_pos;          /* form 1 (pool == NULL): n_points x 3 */
  rgbl_map_points* pool;           /* form 2: slots of a pool on the matcher's device, each at most once */
  const int32_t* slot;
  int n_edges;                     /* 0 .. 2^20, in the order the reference creates them (:160-262) */
  const int32_t* edge_point;       /* non-decreasing */
  const int32_t* edge_cam;         /* a (point, camera) pair at most once */
  const float* edge_obs;           /* n_edges x 3: kpUn.pt.x, kpUn.pt.y, mvuRight (< 0: a monocular edge) */
  const float* edge_inv_sigma2;    /* mvInvLevelSigma2[kpUn.octave] */
  int robust;                      /* bRobust (:177, :209): 1 = Huber with sqrt(5.99) / sqrt(7.815); 0 = no kernel */
  int max_iterations;              /* nIterations: 5, 10 or 20 upstream */
  const volatile int32_t* stop;    /* pbStopFlag (NULL: none), read where g2o's terminate() reads it */
  int stop_after_polls;            /* for tests: N > 0 makes the flag read as set from the N-th poll on */
  const volatile uint8_t* stop_byte; /* the same flag as a one-byte C++ bool (NULL: none) */
} rgbl_ba_input;
typedef struct {
  float* cam_q;                    /* n_cams x 4: what :295 / :299 read, x y z w (the estimate cast to float) */
  float* cam_t;                    /* n_cams x 3 */
  float* point;                    /* n_points x 3: what :377 / :382 read */
  uint8_t* included;               /* n_points: !vbNotIncludedMP (:266-270) - the point has an edge */
  double* chi2;                    /* n_edges: e->chi2() of the last TRIED step (0 if never computed) */
  rgbl_lba_diag diag;              /* ran is always 1 */
} rgbl_ba_output;
/* Host pointers, synchronous; every launch goes on the matcher's stream.  A camera that is flagged fixed or has no edge, and
 * a point without an edge, are not active and come back as the float -> double -> float round trip of their input.  A stop
 * flag that is set on entry is NOT an early return: optimize() runs and ends at its first poll (diag.polls = 1, no
 * iteration), and every output is written.  No fixed camera at all is valid too: g2o then optimises with the gauge free, and
 * so does this call (Levenberg's lambda keeps the reduced system positive definite, or the factorisation fails as csrc/lm_math.h
 * says).  With a pool the optimised positions are also written into the slots.
 * RGBL_ERR_INVALID, before anything is launched and with every output untouched: n_cams outside [0, 2048]; more than 1024
 * active cameras (free and with an edge; the reduced system has 6 per camera) or more than 1024 fixed ones; n_points or
 * n_edges outside their range; more than 2^27 pairs of edges that share a point; edge_point / edge_cam out of range;
 * edge_point decreasing; a repeated (point, camera) pair; a pose, K or bf that is not finite; a slot outside the pool or
 * listed twice; a pool on another device than the matcher; a missing array.  RGBL_ERR_HIP when the device cannot hold the
 * call (the reduced matrix alone is 151 MB at 1024 active cameras): nothing is written. */
int rgbl_bundle_adjustment(rgbl_matcher* h, const rgbl_ba_input* in, rgbl_ba_output* out);
/* The same call evaluated by the HOST build (no device, no handle): the same bits.  pool must be NULL.  Its solve is cubic in
 * the number of active cameras and runs on one core. */
int rgbl_bundle_adjustment_host(const rgbl_ba_input* in, rgbl_ba_output* out);

/* ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12,
 * int windowSize)    /root/reference/include/ORBmatcher.h:72, src/ORBmatcher.cc:648-763 (Tracking::MonocularInitialization,
 * src/Tracking.cc:2526; not on the RGB-L / stereo path - built so that every search routine of ORBmatcher has a device form).
 * Level-0 features of F1 look for their best / second-best F2 feature of level 0 inside a window around vbPrevMatched; a
 * feature takes a candidate over from an earlier one when it is strictly closer (vMatchedDistance), rotation histogram. */
typedef struct {
  int n1;                     /* F1.mvKeysUn.size() (< 2^20) */
  const int32_t* kp1_octave;  /* F1.mvKeysUn[i].octave (>= 0) */
  const float* kp1_angle;     /* F1.mvKeysUn[i].angle */
  const uint8_t* desc1;       /* F1.mDescriptors */
  int n2;                     /* F2.mvKeysUn.size() (<= 65535) */
  const float* kp2_xy;        /* F2.mvKeysUn[i].pt */
  const int32_t* kp2_octave;
  const float* kp2_angle;
  const uint8_t* desc2;       /* F2.mDescriptors */
  float grid[6];              /* Frame::mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv */
  int window_size;
  float nnratio;              /* mfNNratio */
  int check_orientation;      /* mbCheckOrientation */
} rgbl_initialization_input;
/* Host pointers, synchronous.  prev_matched (2 floats per F1 feature) = vbPrevMatched, read as the window centres and
 * updated for the matched features like the reference does; matches12 (n1 entries) = vnMatches12; *out_nmatches = the
 * return value. */
int rgbl_search_for_initialization(rgbl_matcher* h, const rgbl_initialization_input* in, float* prev_matched, int32_t* matches12,
                                   int* out_nmatches);

/* ------------------------------------------------------------------------------------------------
 * ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>)    SURVEY.md 8(f) row f4
 *   replaces the per-feature descent of Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:828-835,
 *   src/KeyFrame.cc:98-107: mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)),
 *   Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1255, FORB.cpp:79-98.  The tree lives on the device.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rgbl_vocabulary rgbl_vocabulary;
/* ORBVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1425; System.cc:115): the ORBvoc.txt format. */
int rgbl_vocabulary_load_text(const char* path, int device, rgbl_vocabulary** out);
/* The same from flat arrays: node 0 = root, children of node i = child[child_off[i] .. child_off[i+1]) in file order,
 * 32-byte node descriptors, Node::weight, Node::word_id (leaves). */
int rgbl_vocabulary_create(int n_nodes, int L, const int32_t* child_off, const int32_t* child, const uint8_t* desc,
                           const double* weight, const int32_t* word_id, int device, rgbl_vocabulary** out);
void rgbl_vocabulary_destroy(rgbl_vocabulary* v);
int rgbl_vocabulary_info(const rgbl_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words);
/* transform(features, BowVector, FeatureVector, levelsup).  Host pointers, synchronous.  BowVector as ascending word ids +
 * values (TF-IDF, L1-normalised doubles), FeatureVector as ascending node ids + CSR offsets (n_nodes + 1) + feature
 * indices (ascending inside a node).  RGBL_ERR_CAPACITY when cap_words / cap_nodes (n is always enough) are too small. */
int rgbl_bow_transform(rgbl_vocabulary* v, const uint8_t* desc, int n, int levelsup, uint32_t* word_id, double* word_val,
                       int cap_words, int* n_words, uint32_t* node_id, int32_t* node_off, uint32_t* node_feat, int cap_nodes,
                       int* n_nodes);
/* The same on a frame whose descriptors are resident (rgbl_device_frame): nothing is uploaded. */
int rgbl_bow_transform_frame(rgbl_vocabulary* v, const rgbl_device_frame* frame, int levelsup, uint32_t* word_id, double* word_val,
                             int cap_words, int* n_words, uint32_t* node_id, int32_t* node_off, uint32_t* node_feat, int cap_nodes,
                             int* n_nodes);
/* Device-resident batch, descent only: the descriptors of rgbl_extract_batch_device() (frame b at d_desc + b*cap*32, d_n
 * counts) -> per feature word id, word weight, node id at level L - levelsup.  Enqueued on hip_stream (NULL: own stream). */
int rgbl_bow_descend_batch_device(rgbl_vocabulary* v, void* hip_stream, const uint8_t* d_desc, const int32_t* d_n, int batch,
                                  int cap, int levelsup, int32_t* d_word, double* d_weight, int32_t* d_node);

/* F12 with the reference's fp32 evaluation order (Pinhole.cpp:109-112); K = {fx, fy, cx, cy}. Host. */
void rgbl_fundamental(const float K1[4], const float K2[4], const float R12[9], const float t12[3],
                      float F12[9]);

/* ------------------------------------------------------------------------------------------------
 * Host-fed batches      Frame::Frame(imGray, PointCloud, ...) (src/Frame.cc:289-377) + Tracking::GrabImageRGBL
 *                       (src/Tracking.cc:1563-1582) for batches of frames that arrive in host memory, one after another,
 *                       the way Examples/RGB-L/rgbl_kitti.cc:87-94, 151-185 reads them (colour PNG + velodyne .bin scan)
 * ----------------------------------------------------------------------------------------------
 * A feeder sits on an existing extractor handle and depth handle (it keeps no configuration of theirs) and streams batches
 * through `slots` page-locked slots, in ring order:
 *
 *   rgbl_feeder_acquire(f, &slot);                        the next slot; its previous batch must have been collected
 *   for b in 0 .. batch - 1:
 *     rgbl_feeder_scan(f, slot, b, n_b, &xyzi);           reserves n_b .bin records (a .bin file's size / 16) for frame b
 *     rgbl_feeder_image(f, slot, b, &px);                 w x h x channels bytes, row stride w * channels
 *     ... fread / decode straight into xyzi and px        (any thread, any frame, once its scan is reserved)
 *   rgbl_feeder_submit(f, slot, batch);                   queues the batch and returns at once
 *   ... acquire / fill / submit the next slots ...
 *   rgbl_feeder_collect(f, slot, &res);                   waits for that batch only; host pointers to its results
 *
 * Slot memory: one page-locked block (hipHostMalloc) per slot holding max_batch images, max_points_batch packed scan records,
 *   the scan offsets and the page-locked copies of the results.  Nothing is copied twice on the host.
 * Scan reservation: in frame order b = 0, 1, ... from one thread (the scans are packed back to back); over-reserving
 *   (more than max_points in one scan, more than max_points_batch in the batch, b out of order) returns RGBL_ERR_CAPACITY
 *   resp. RGBL_ERR_INVALID.  After that any thread may fill any frame of the slot.  An empty scan (n = 0) is valid.
 * Submit: on the feeder's own copy stream one host-to-device copy each of the images, of the scan records in use and of the
 *   offsets, each behind the last readers of the slot's device buffers (events).  Then, ordered by events: cv::cvtColor
 *   (Tracking.cc:1567-1580; channels 1 extracts straight from the slot) and ORBextractor::operator() on the extractor's
 *   stream, UndistortKeyPoints (Frame.cc:837-845, only when n_dist > 0 and dist[0] != 0), the projection of the scans
 *   (rgbl_depth_project_xyzi_varlen_batch_device) on the depth stream next to the extraction, the keypoint gather
 *   (DepthModule.cc:82-104) and the copy of the results into the slot's page-locked block - also on the depth stream: the
 *   copy stream carries only the NEXT batches' inputs, which would otherwise wait for this batch's kernels.
 * Results (rgbl_feeder_results): the layout of rgbl_extract_batch with cap = rgbl_extractor_max_keypoints(ex): frame b's
 *   keypoints at kp + b * cap, descriptors at desc + b * cap * 32, mvDepth / mvuRight at depth / uright + b * cap, mvKeysUn
 *   (x, y) at kpun_xy + b * cap * 2 (NULL without undistortion: mvKeysUn = mvKeys), n / mono: batch ints.  Valid until the
 *   slot is acquired again.
 * Errors: RGBL_ERR_INVALID for acquiring a slot whose batch was submitted and not collected (or is still being filled),
 *   collecting a slot that holds no submitted batch (collecting twice), submitting a batch whose scans were not all reserved
 *   or that is longer than max_batch, and for a configuration that does not fit its handles.  Deferred device errors surface
 *   in collect (the results are filled all the same): RGBL_ERR_OVERFLOW / RGBL_ERR_CAPACITY of the extractor, as
 *   rgbl_extractor_sync reports them, and RGBL_ERR_OVERFLOW for a scan the projection could not hold.  They belong to the
 *   collected batch: the flags are taken and cleared on the device right behind that batch's own extraction and projection.
 *   A submit that fails after it has queued part of the batch leaves the slot failed: collect waits for what was queued and
 *   returns that error (no results); the slot can then be acquired again.
 * A feeder drives its handles' streams: while it lives, the handles serve no other caller.  Nothing of a handle changes when
 * no feeder drives it. */
typedef struct rgbl_feeder rgbl_feeder;
typedef struct {
  int channels, blue_first;        /* 1 gray, 3 / 4 interleaved; blue_first = settings Camera.RGB == 0 (BGR, as cv::imread) */
  int max_batch;                   /* frames per batch, <= both handles' max_batch */
  int max_points;                  /* points per scan, <= the depth handle's max_points */
  long long max_points_batch;      /* points per batch (packed scan records per slot); 0 = max_batch * max_points */
  int slots;                       /* batches in flight, >= 2 */
  float K[4];                      /* fx, fy, cx, cy (undistortion only) */
  float dist[5];                   /* k1, k2, p1, p2[, k3] */
  int n_dist;                      /* 0, 4 or 5; 0 or dist[0] == 0: no undistortion (Frame.cc:839) */
} rgbl_feeder_cfg;
typedef struct {
  int batch, cap;
  const rgbl_keypoint* kp;         /* batch x cap */
  const uint8_t* desc;             /* batch x cap x 32 */
  const int32_t* n;                /* batch */
  const int32_t* mono;             /* batch: ORBextractor::operator()'s return value */
  const float* depth;              /* batch x cap: mvDepth (-1 = none) */
  const float* uright;             /* batch x cap: mvuRight */
  const float* kpun_xy;            /* batch x cap x 2: mvKeysUn, NULL without undistortion */
} rgbl_feeder_results;
int rgbl_feeder_create(const rgbl_feeder_cfg* cfg, rgbl_extractor* ex, rgbl_depth* dm, rgbl_feeder** out);
void rgbl_feeder_destroy(rgbl_feeder* f);  /* waits for the batches in flight */
int rgbl_feeder_acquire(rgbl_feeder* f, int* slot);
int rgbl_feeder_image(rgbl_feeder* f, int slot, int b, uint8_t** px);
int rgbl_feeder_scan(rgbl_feeder* f, int slot, int b, int n, float** xyzi);
int rgbl_feeder_submit(rgbl_feeder* f, int slot, int batch);
int rgbl_feeder_collect(rgbl_feeder* f, int slot, rgbl_feeder_results* out);
/* The same arrays on the device, for work that goes on there (Hamming matchers, rgbl_gather_pack, rgbl_device_frame_capture):
 * *done_event (a HIP event) fires when they are complete; wait for it with rgbl_event_wait.  Valid from submit until the slot's
 * next batch is submitted; the slot must still be collected before it is acquired again.  The feeder does not know the device
 * work a caller queues on its own streams: that work must have COMPLETED (rgbl_*_sync, or an event the caller waits for on the
 * host) before the caller acquires the slot again, because the next submit overwrites these arrays. */
int rgbl_feeder_device_outputs(rgbl_feeder* f, int slot, rgbl_feeder_results* out, void** done_event);
/* Page-locked bytes the feeder holds (all slots). */
long long rgbl_feeder_pinned_bytes(const rgbl_feeder* f);

/* ------------------------------------------------------------------------------------------------
 * KeyFrameDatabase      the BoW place-recognition queries of src/KeyFrameDatabase.cc
 *   add / erase / clear / clearMap (:39-98) and the part of the two Detect* functions the reference calls that depends on
 *   nothing but BowVectors:
 *     DetectRelocalizationCandidates (:733-790; caller Tracking::Relocalization, src/Tracking.cc:3651)
 *     DetectNBestCandidates          (:604-669; caller LoopClosing::NewDetectCommonRegions, src/LoopClosing.cc:491)
 *   i.e. lKFsSharingWords with mn*Words (:615-635, :741-756), maxCommonWords and minCommonWords = int(max * 0.8f) (:641-648,
 *   :762-769), and mpVoc->score() = L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) of the key frames with
 *   more than minCommonWords common words (:655-666, :776-787).  The covisibility accumulation and the selection (:671-729,
 *   :792-844) read GetBestCovisibilityKeyFrames / GetMap / isBad of the caller's objects and stay with the caller
 *   (orb_slam3_rgbl_amd/shim/KeyFrameDatabase.h, frontend.KeyFrameDatabase).  DetectLoopCandidates, DetectCandidates and
 *   DetectBestCandidates have no caller in the reference and are not provided.
 * ----------------------------------------------------------------------------------------------
 * The stored BowVectors live in an append-only device arena that doubles when it is full; erased key frames leave tombstones
 * and the arena is compacted once more than half of its words are dead.  Neither changes any query result.  Every entry point
 * takes the handle's own mutex (the reference's mMutex: add comes from loop closing, erase from KeyFrame::SetBadFlag, the
 * queries from tracking) and works on the handle's own stream.
 *
 * Order: every add gets the next sequence number - the key frame's position in every inverted list it joins in the reference
 * (list::push_back, :44).  Erasing a key frame and adding it again puts it at the end.  A query returns lKFsSharingWords in
 * the reference's first-encounter order: ascending by (smallest common word id, sequence number), which is what walking the
 * query's words in ascending order and each list front to back produces. */
typedef struct rgbl_kf_database rgbl_kf_database;
int rgbl_kfdb_create(int device, int n_vocab_words, rgbl_kf_database** out);
void rgbl_kfdb_destroy(rgbl_kf_database* db);
/* KeyFrameDatabase::add: the ascending word ids and values of rgbl_bow_transform*.  RGBL_ERR_INVALID for ids that do not
 * ascend or are >= n_vocab_words, and for a kf_id that is in the database already (the reference would push it into its lists
 * a second time and count every word twice; no caller of the reference does that). */
int rgbl_kfdb_add(rgbl_kf_database* db, int64_t kf_id, int32_t map_id, int n_words, const uint32_t* word_id, const double* word_val);
/* erase (:47-66; a key frame that is not stored: nothing happens), clear (:68-72), clearMap (:74-98). */
int rgbl_kfdb_erase(rgbl_kf_database* db, int64_t kf_id);
int rgbl_kfdb_clear(rgbl_kf_database* db);
int rgbl_kfdb_clear_map(rgbl_kf_database* db, int32_t map_id);
/* KeyFrame::UpdateMap: a stored key frame moves to another map (LoopClosing.cc:1527, :1736, :1898 after a merge).  clearMap tests
 * GetMap() when it runs (:87), so rgbl_kfdb_clear_map goes by the id set last.  Its place in the order does not change.
 * A key frame that is not stored: nothing happens. */
int rgbl_kfdb_set_map(rgbl_kf_database* db, int64_t kf_id, int32_t map_id);
/* stored key frames and the words they hold */
int rgbl_kfdb_size(rgbl_kf_database* db, int* n_alive, long long* n_words);
/* A test aid, not part of the reference's interface - the arena: words in use (tombstones included), capacity in words, entry slots (tombstones included), compactions so far */
int rgbl_kfdb_arena_info(rgbl_kf_database* db, long long* used_words, long long* cap_words, int* n_slots, int* n_compactions);

typedef struct {
  int n_words;                    /* the query's BowVector: ascending ids, values */
  const uint32_t* word_id;
  const double* word_val;
  int n_excluded;                 /* key frames that are no shared entries and do not count towards the maximum:           */
  const int64_t* excluded_kf;     /*   DetectNBestCandidates passes pKF->GetConnectedKeyFrames() (:613, :626); NULL / 0 else */
  int min_words_floor;            /* minCommonWords = max(int(maxCommonWords * 0.8f), min_words_floor); 0 for both callers  */
} rgbl_kfdb_query_input;
typedef struct {
  int cap;                        /* room in the four arrays */
  int64_t* share_kf;              /* lKFsSharingWords, in the reference's order                                            */
  int32_t* share_words;           /* mnRelocWords / mnPlaceRecognitionWords of that key frame                              */
  float* share_score;             /* mRelocScore / mPlaceRecognitionScore where scored[i]; NOT written where it is 0       */
  uint8_t* scored;                /* share_words[i] > min_common_words                                                     */
  int n_share, max_common_words, min_common_words;
} rgbl_kfdb_query_output;
/* Host pointers, synchronous.  Every key frame that shares a word is returned, not only the scored ones: the covisibility
 * step reads mn*Query and the (possibly stale) m*Score of neighbours below the threshold (:686-690, :807-811), so a caller
 * has to stamp all of them.  RGBL_ERR_CAPACITY, with n_share set and no array written, when cap < n_share.  Queries hold at
 * most 15360 words. */
int rgbl_kfdb_query(rgbl_kf_database* db, const rgbl_kfdb_query_input* in, rgbl_kfdb_query_output* out);
/* n_queries queries in one launch over (query, entry); rgbl_kfdb_query is its n_queries = 1 case.  Query q's words are
 * word_id / word_val[word_off[q] .. word_off[q+1]), its excluded key frames excl_kf[excl_off[q] .. excl_off[q+1]) (excl_off
 * NULL: none), its floor min_words_floor[q] (NULL: 0); its results go to row q of the n_queries x cap arrays and to entry q
 * of n_share / max_common_words / min_common_words.  RGBL_ERR_CAPACITY if any row is too small (the other rows are filled).  At most
 * 65535 queries per call (RGBL_ERR_INVALID beyond). */
int rgbl_kfdb_query_batch(rgbl_kf_database* db, int n_queries, const int32_t* word_off, const uint32_t* word_id,
                          const double* word_val, const int32_t* excl_off, const int64_t* excl_kf,
                          const int32_t* min_words_floor, int cap, int64_t* share_kf, int32_t* share_words, float* share_score,
                          uint8_t* scored, int32_t* n_share, int32_t* max_common_words, int32_t* min_common_words);
/* A measurement aid (tools/kfdb_bench.py): per-kernel times of the queries (HIP events), as rgbl_matcher_profile / _profile_read */
int rgbl_kfdb_profile(rgbl_kf_database* db, int enable);
int rgbl_kfdb_profile_read(rgbl_kf_database* db, const char** names, double* total_ms, long* launches, int cap);

/* ------------------------------------------------------------------------------------------------
 * Environment switches.  Every one of them is read ONCE, when the handle it concerns is created (never on a launch path:
 * the entry points are called from the three SLAM threads), and is a tuning / test aid - the defaults are what is measured
 * and shipped.  Results are bit-identical under all of them (parity_checks.check_switches: the batch and the single-frame
 * extraction and the Hamming scan under every switch that changes a launch path, on the emulator and on the MI355X).
 *
 *   rgbl_extractor_create
 *     RGBL_SPLIT_PYR=k      batches: the pyramid levels k .. L-1 and their FAST cells leave the main launch chain for the auxiliary
 *                           stream (default L / 2 from 6 levels on; 0 = off)
 *     RGBL_LEVEL_SPLIT=k    single frames: the levels 1 .. k-1 get a stream of their own (default 3; 0 = off)
 *     RGBL_FAST_BS=64|128   waves per FAST detection cell (default: 64 for batches of >= 8 frames, 128 for single frames)
 *     RGBL_COMPACT=0|1      k_compact_cells never / always (default: batches of >= 8 frames)
 *     RGBL_DENSE=0          quad-tree reads the cells' own slots instead of a dense per-level candidate list
 *     RGBL_OCTREE_NCAP=0|512|2048   quad-tree node capacity in LDS (0 = the key-moving kernel on global lists; default by nFeatures)
 *     RGBL_OCTREE_WG=256|512        quad-tree workgroup width (default by batch size)
 *     RGBL_OCTREE_LDSKEYS=0         single frames: candidate lists stay in global memory
 *     RGBL_OCTREE_HIST=0            breadth-first rounds as passes over the keys instead of on the per-cell count pyramid
 *     RGBL_OCTREE_STAMPS=1          the quad-tree kernel leaves phase time stamps (rgbl_extractor_debug_stamps)
 *     RGBL_GAUSS_BS=256     four-wave workgroups for the Gaussian (default two waves)
 *     RGBL_XCD_MAP=0        plain (items, frames) grids instead of the XCD-aware (8, items, frames / 8) mapping (also rgbl_depth_create, rgbl_rectifier_create, rgbl_resizer_create)
 *     RGBL_GRAPH=0          host-pointer extraction without hipGraph replay
 *   rgbl_depth_create
 *     RGBL_DEPTH_MAX_GEN=n  generations of the index map before it is cleared (tests of the wrap-around)
 *   rgbl_matcher_create
 *     RGBL_BF_MFMA=0|i8     Hamming scan on the VALU (popcount) / on v_mfma_i32_32x32x32_i8 (default: block-scaled FP4 instruction)
 *     RGBL_BF_SPLIT=0       one pair per call without train-set slices
 *     RGBL_GBA_PANEL=16|64  rgbl_bundle_adjustment: columns per panel of the reduced system's solve (32; the bits do not depend on it)
 *   first allocation of the process (whatever handle makes it)
 *     RGBL_ALLOC_FILL=0..255   TEST switch: every device and page-locked block the library allocates is filled with that byte before
 *                           its first use, the grow-only staging blocks (the matcher's arena and mirror, the pool's, vocabulary's and
 *                           stereo matcher's stages) before every call that reuses them; unset: one cached branch per allocation
 *   first rgbl_comm_* call
 *     RGBL_RCCL_LIB=path    librccl to dlopen when none is mapped into the process yet
 * ---------------------------------------------------------------------------------------------- */

#ifdef __cplusplus
}
#endif
#endif /* RGBL_FRONTEND_H */
