// matcher_call.h — the scaffold of one host-pointer call on a matcher handle, shared by matcher.hip, optimize.hip, ransac.hip
// and lba.hip: the handle and the map-point pool as the entry points see them, the call's one-upload / one-readback staging
// (HostCall, put_features), the pool prologue (PoolCall), the timed launch and the element-wise device test hook.
// Private to csrc (not exported); included after common.h.
#pragma once

#include <string.h>

#include <algorithm>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "common.h"

// ---- rgbl_map_points: map-point data resident on the device ------------------------------------------------------------
// One allocation: world_pos [cap x 3] | normal [cap x 3] | min [cap] | max [cap] | desc [cap x 32], every array 256-byte
// aligned (64 bytes per slot).  `mu` is held by every call that reads or writes the arrays until its device work is done.
struct rgbl_map_points {
  int device = 0, cap = 0;
  std::mutex mu;
  uint8_t* block = nullptr;
  float *d_wpos = nullptr, *d_normal = nullptr, *d_min = nullptr, *d_max = nullptr;
  uint8_t* d_desc = nullptr;
  hipStream_t stream = nullptr;
  uint8_t *d_stage = nullptr, *h_stage = nullptr;   // one update's packed arrays and their page-locked mirror (grow-only)
  size_t stage_size = 0;
};

struct rgbl_matcher {
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;
  rgbl::KernelTimer timer;
  uint8_t* d_buf = nullptr;  // grow-only staging arena for the host entry points
  size_t buf_size = 0;
  uint8_t* h_pin = nullptr;  // grow-only page-locked mirror of the brute-force scan's inputs / outputs (rgbl_hamming_bf)
  size_t pin_size = 0;
  // tuning switches, read ONCE at rgbl_matcher_create (include/rgbl_frontend.h lists them): never on a launch path
  bool bf_matrix = true;   // RGBL_BF_MFMA=0: the VALU popcount scan (k_hamming_bf)
  bool bf_fp4 = true;      // RGBL_BF_MFMA=i8: v_mfma_i32_32x32x32_i8 (k_hamming_mfma) instead of the block-scaled FP4 instruction
  bool bf_split = true;    // RGBL_BF_SPLIT=0: one pair per call without train-set slices
  int gba_panel = 32;      // RGBL_GBA_PANEL=16|64: the panel width of the global bundle adjustment's solve (gba.hip); the bits do not depend on it
};

namespace rgbl {

constexpr int kProjMaxLevels = 16;   // pyramid levels a call may name (the projection searches, the optimisers, MLPnP)

inline int ensure_arena(rgbl_matcher* m, size_t bytes) {
  if (bytes <= m->buf_size) return RGBL_OK;
  if (m->d_buf) { RGBL_HIP(hipStreamSynchronize(m->stream)); RGBL_HIP(hipFree(m->d_buf)); m->d_buf = nullptr; m->buf_size = 0; }
  const size_t sz = std::max(bytes, (size_t)1 << 20);
  RGBL_HIP(rgbl::device_alloc(&m->d_buf, sz));
  m->buf_size = sz;
  return RGBL_OK;
}
inline int ensure_pin(rgbl_matcher* m, size_t bytes) {
  if (bytes <= m->pin_size) return RGBL_OK;
  if (m->h_pin) { (void)hipHostFree(m->h_pin); m->h_pin = nullptr; m->pin_size = 0; }
  const size_t sz = std::max(bytes, (size_t)1 << 20);
  RGBL_HIP(rgbl::pinned_alloc(&m->h_pin, sz));
  m->pin_size = sz;
  return RGBL_OK;
}
// One call of a host-pointer entry point.  The device arena and its page-locked mirror share ONE layout: what the call
// uploads is copied into the mirror at the offsets its device copies have and goes up with ONE hipMemcpyAsync (round 5
// queued one per array, 8 - 17 per call, from pageable memory); the result arrays are taken back to back and come back
// with one.  Arrays of a frame that is resident on the device (rgbl_device_frame) are not staged at all.
// begin() runs the call's layout - its put / put_fill / stage / result / scratch calls - twice: a measuring pass that copies,
// waits for and launches nothing, then, with the arena and mirror grown to that size, the carving pass.
struct HostCall {
  rgbl_matcher* m;
  hipStream_t s;
  bool carving = false;
  size_t off = 0, up_end = 0, res_begin = ~(size_t)0, res_end = 0;
  explicit HostCall(rgbl_matcher* mm) : m(mm), s(mm->stream) {}
  template <class Layout> int begin(Layout&& layout) {   // ... and the call's ONE upload
    RGBL_TRY(layout());
    const size_t measured = off;
    RGBL_TRY(ensure_arena(m, measured));
    RGBL_TRY(ensure_pin(m, measured));
    RGBL_HIP(refill_staging(m->d_buf, m->h_pin, measured, s));   // RGBL_ALLOC_FILL: what the last call left behind is gone
    carving = true;
    off = up_end = 0;
    RGBL_TRY(layout());
    if (off != measured) { set_error("staging layout: %zu bytes measured, %zu carved", measured, off); return RGBL_ERR_INVALID; }
    if (up_end) RGBL_HIP(hipMemcpyAsync(m->d_buf, m->h_pin, up_end, hipMemcpyHostToDevice, s));
    return RGBL_OK;
  }
  template <class E> E* take(size_t count) {   // every array starts 256-byte aligned; nullptr while measuring
    off = (off + 255) / 256 * 256;
    E* p = carving ? reinterpret_cast<E*>(m->d_buf + off) : nullptr;
    off += count * sizeof(E);
    return p;
  }
  size_t off_of(const void* d) const { return (size_t)(reinterpret_cast<const uint8_t*>(d) - m->d_buf); }
  template <class E> void put(const E** dst, const E* src, size_t count) {
    E* p = take<E>(count);
    *dst = p;
    if (carving && count) memcpy(m->h_pin + off_of(p), src, count * sizeof(E));
    up_end = off;
  }
  template <class E> E* put_fill(size_t count, int byte) {   // an array the device starts from (e.g. all -1) travels with the upload
    E* p = take<E>(count);
    if (carving && count) memset(m->h_pin + off_of(p), byte, count * sizeof(E));
    up_end = off;
    return p;
  }
  template <class E, class Fill> E* stage(size_t count, Fill fill) {   // fill(mirror) writes the upload itself
    E* p = take<E>(count);
    if (carving) fill(reinterpret_cast<E*>(m->h_pin + off_of(p)));
    up_end = off;
    return p;
  }
  template <class E> E* scratch(size_t count) { return take<E>(count); }
  template <class E> void mark_result(E* p, size_t count) {
    if (!carving) return;
    res_begin = std::min(res_begin, off_of(p));
    res_end = std::max(res_end, off_of(p) + count * sizeof(E));
  }
  template <class E> E* result(size_t count) { E* p = take<E>(count); mark_result(p, count); return p; }
  int fetch() {   // the call's only wait
    if (res_end > res_begin) RGBL_HIP(hipMemcpyAsync(m->h_pin + res_begin, m->d_buf + res_begin, res_end - res_begin, hipMemcpyDeviceToHost, s));
    RGBL_HIP(hipStreamSynchronize(s));
    m->timer.collect();
    return RGBL_OK;
  }
  template <class E> const E* host(const E* d) const { return reinterpret_cast<const E*>(m->h_pin + off_of(d)); }
  // a frame's resident arrays: the stream waits for whatever filled them last
  int use(const rgbl_device_frame* f, int n) {
    if (f->device != m->device || f->n != n) { set_error("device frame: %d features on device %d, the call says %d on device %d", f->n, f->device, n, m->device); return RGBL_ERR_INVALID; }
    if (carving) RGBL_HIP(hipStreamWaitEvent(s, f->ready, 0));
    return RGBL_OK;
  }
};

// A frame's per-feature arrays that the call reads (a null destination: not read): the resident copy when the frame has one
// (dev), else staged with the rest of the call's upload.
inline int put_features(HostCall& hc, const rgbl_device_frame* dev, int n, const uint8_t* desc, const float* xy, const int32_t* oct,
                 const float* ur, const uint8_t** d_desc, const float** d_xy, const int32_t** d_oct, const float** d_ur) {
  if (dev) {
    RGBL_TRY(hc.use(dev, n));
    if (d_desc) *d_desc = dev->d_desc;
    if (d_xy) *d_xy = dev->d_xy;
    if (d_oct) *d_oct = dev->d_oct;
    if (d_ur) *d_ur = dev->d_ur;
    return RGBL_OK;
  }
  if (d_desc) hc.put(d_desc, desc, (size_t)n * 32);
  if (d_xy) hc.put(d_xy, xy, (size_t)n * 2);
  if (d_oct) hc.put(d_oct, oct, (size_t)n);
  if (d_ur) hc.put(d_ur, ur, (size_t)n);
  return RGBL_OK;
}

// The correspondences of a problem that pairs the features of a frame with map points (pose optimisation, MLPnP): mp_index[i]
// is feature i's point, or -1.  check_correspondences refuses, in feature order, an index outside [-1, n_points) and - for a
// frame given as host arrays (octave non-null) - a paired feature's octave outside [0, n_levels), and counts the pairs; `what`
// and b name the caller's problem in the error texts.  list_correspondences writes each pair's feature and its point's row of
// the map side: the pool's slot (slot non-null) or the index itself.
inline int check_correspondences(const char* what, int b, int n, const int32_t* mp_index, int n_points, const int32_t* octave, int n_levels, int* count) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const int p = mp_index[i];
    if (p < -1 || p >= n_points) { set_error("%s %d: mp_index[%d] = %d outside [-1, %d)", what, b, i, p, n_points); return RGBL_ERR_INVALID; }
    if (p < 0) continue;
    ++m;
    if (octave && (octave[i] < 0 || octave[i] >= n_levels)) { set_error("%s %d: octave %d of feature %d outside [0, %d)", what, b, octave[i], i, n_levels); return RGBL_ERR_INVALID; }
  }
  *count = m;
  return RGBL_OK;
}
inline void list_correspondences(int n, const int32_t* mp_index, const int32_t* slot, int32_t* feat, int32_t* point) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const int p = mp_index[i];
    if (p < 0) continue;
    feat[k] = i;
    point[k] = slot ? slot[p] : p;
    ++k;
  }
}

// One kernel launch of a call on stream s inside the handle's timer bracket (the names are what bench.py and
// tools/extract_kernel_times.py read), `lds` bytes of dynamic LDS; a launch the runtime refuses is the call's error.
template <class... Params, class... Args>
int launch(rgbl_matcher* m, hipStream_t s, const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, const Args&... args) {
  m->timer.begin(name, s);
  hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
  m->timer.end(s);
  RGBL_HIP(hipGetLastError());
  return RGBL_OK;
}

// The prologue of the batch entry points whose problems read resident frames and a map-point pool: the problems of one call
// share one pool, pool and frames are on the matcher's device, and the pool is locked while its slots are range-checked and
// until the call returns.  An entry point declares its PoolCall FIRST, then - after lock() - StreamDrain, then HostCall:
// destruction runs backwards, so the stream is drained (error returns included) before the pool is released.
struct PoolCall {
  const rgbl_matcher* m;
  const char *what, *frame;   // the entry point and a resident frame as the error texts name them
  rgbl_map_points* pool = nullptr;
  std::unique_lock<std::mutex> held;
  PoolCall(const rgbl_matcher* matcher, const char* name, const char* frame_name) : m(matcher), what(name), frame(frame_name) {}
  // "sim3 3:" names problem 3 of a batch; an entry point that is one problem passes b = -1 and is named alone
  std::string who(int b) const { return b < 0 ? std::string(what) : std::string(what) + " " + std::to_string(b); }
  // problem b reads pool `p` and the resident `frames` (null: host arrays)
  int note(rgbl_map_points* p, std::initializer_list<const rgbl_device_frame*> frames, int b) {
    for (const rgbl_device_frame* fr : frames)
      if (fr && fr->device != m->device) {
        set_error("%s: %s is on device %d, the matcher on %d", who(b).c_str(), frame, fr->device, m->device);
        return RGBL_ERR_INVALID;
      }
    if (!p) return RGBL_OK;
    if (pool && pool != p) { set_error("%s: the problems of one call share one pool", who(b).c_str()); return RGBL_ERR_INVALID; }
    pool = p;
    if (pool->device != m->device) { set_error("%s: the pool is on device %d, the matcher on %d", who(b).c_str(), pool->device, m->device); return RGBL_ERR_INVALID; }
    return RGBL_OK;
  }
  // locks the pool; under the lock, check(b) asks holds() for every slot problem b names (none if it does not read the pool)
  // and returns RGBL_OK, or sets the error text of the first slot outside and returns RGBL_ERR_INVALID
  int lock(int B, const std::function<int(int)>& check) {
    if (!pool) return RGBL_OK;
    held = std::unique_lock<std::mutex>(pool->mu);
    for (int b = 0; b < B; ++b) RGBL_TRY(check(b));
    return RGBL_OK;
  }
  bool holds(int slot) const { return slot >= 0 && slot < pool->cap; }
};

// The element-wise device test hooks (rgbl_test_*_device): every array of `in` (n elements each) goes to the device,
// launch(d_in, d_out, grid, block) runs one work-item per element on the null stream, d_out comes back as `out`.  The device
// arrays are freed on every path.
template <class T, class Launch> int elementwise_device_hook(std::initializer_list<const T*> in, T* out, int n, Launch launch) {
  const size_t bytes = sizeof(T) * (size_t)n;
  std::vector<T*> d(in.size() + 1, nullptr);   // the inputs, then the output
  hipError_t e = hipSuccess;
  for (T*& p : d)
    if (e == hipSuccess) e = rgbl::device_alloc(reinterpret_cast<void**>(&p), bytes);
  size_t k = 0;
  for (const T* h : in) {
    if (e == hipSuccess) e = hipMemcpy(d[k], h, bytes, hipMemcpyHostToDevice);
    ++k;
  }
  if (e == hipSuccess) {
    launch(d.data(), d.back(), dim3((unsigned)((n + 255) / 256)), dim3(256));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d.back(), bytes, hipMemcpyDeviceToHost);
  for (T* p : d)
    if (p) (void)hipFree(p);
  if (e != hipSuccess) { set_error("device test hook: %s", hipGetErrorString(e)); return RGBL_ERR_HIP; }
  return RGBL_OK;
}

}  // namespace rgbl
