// resize.hip — the image resize in front of cvtColor: cv::resize(im, imToFeed, settings_->newImSize()) of System::TrackStereo /
// TrackRGBD / TrackRGBL / TrackMonocular (src/System.cc:269-271, 349-351, 486-489, 557-560) on 8-bit images with 1, 3 or 4
// interleaved channels, default INTER_LINEAR, any ratio on either axis.  Restated from OpenCV 4.x imgproc/src/resize.cpp
// (parity vs the restatement = the oracle's cv::resize at one channel, unpinned); interleaved channels are the one-channel
// arithmetic per channel (xofs[dx * cn + k] = sx * cn + k, the same two weights for every k):
//   per axis  f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; x only: s < 0 -> (0, 0), s >= sw - 1 -> (sw - 1, 0)
//   weights   cvRound((1 - f) * 2048), cvRound(f * 2048)                       (resize_tab.h: build_resize_tab)
//   h = p0 * a0 + p1 * a1 per source row (rows s, s + 1 clamped into the image)
//   dst = ((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
// At exactly half size OpenCV reroutes INTER_LINEAR to INTER_AREA; on 8-bit images the formula above then IS the 2 x 2 mean
// (a + b + c + d + 2) >> 2 (every weight is 1024, no clamp occurs), so one kernel serves both branches
// (tests/test_resize_restatements.py states the equality).
//
// k_resize_image<C>: a workgroup makes a tile of 64 destination columns x up to kRszRows rows.
//   phase 1  the horizontal pass of the source rows the tile needs (at most kRszSlots, listed by the host: with strong
//            down-scaling the rows between two destination rows are never read) into LDS as 16-bit h >> 4 (<= 32640).  A
//            work-item makes 4 consecutive pixels of a row: their table entries are one 32-byte read, requested before the
//            taps; the taps of a pixel are one 4-byte (C = 1) or 8-byte (C = 3, 4) window read straight from global memory, any
//            alignment, pulled back at the end of a row so that it stays inside it.
//   phase 2  the vertical pass from LDS: the same work-item layout, 4 pixels = one / three / four 32-bit stores (bytes for the
//            partial last group of a row and for destinations that are not 4-byte aligned).
// The host cuts the destination rows into tiles when the handle is created: a tile takes rows while it has fewer than
// kRszRows and its source rows fit kRszSlots - with up-scaling destination rows share source rows, with strong down-scaling
// a tile shrinks to as little as one row (two source rows always fit).  All tables are uploaded once; no call allocates
// except the grow-only staging of the host-pointer call.
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "resize_tab.h"

namespace rgbl {

constexpr int kRszTileW = 64;     // 16 work-items x 4 pixels
constexpr int kRszRows = 32;      // work-item (tid & 15, tid >> 4) owns the rows (tid >> 4) + 16 r, r < kRszPer
constexpr int kRszSlots = 32;     // source rows of a tile in LDS: 64 x C x 2 bytes each, 16 KiB at C = 4
constexpr int kRszPer = 2;
static_assert(kRszRows == 16 * kRszPer && kRszSlots == 16 * kRszPer, "256 work-items, 16 per row");
constexpr int kResizeMaxSide = 16384;

// One destination column at C channels.  win: byte offset of the pixel's window inside a source row (20 bits) | k0 << 20 |
// k1 << 24, the bytes at which the left / right tap start inside the window (k1 = k0 where the right tap's weight is 0: the
// last column).  Sources narrower than a window ("thin") keep win = the left tap's byte, k0 = 0, and are read byte by byte.
struct ResizeX { uint32_t win, wt; };         // wt: a0 | a1 << 16
struct ResizeY { uint32_t slots, wt; };       // slots: LDS slot of row s | slot of row s + 1 << 8 (both clamped); wt: b0 | b1 << 16
struct ResizeRows { int32_t dy0, ndy, nsr, pad; int32_t srow[kRszSlots]; };   // a tile row: destination rows, its source rows

static inline int resize_window_bytes(int C) { return C == 1 ? 4 : 8; }

// grid = xcd_grid(tiles_x * tile rows, B) (common.h), block = 256.  xtab is padded to tiles_x * 64 entries with copies of the
// last one.  words: destination base and strides are multiples of 4.
template <int C>
__global__ __launch_bounds__(256) void k_resize_image(const ResizeRows* __restrict__ tiles, const ResizeX* __restrict__ xtab,
                                                      const ResizeY* __restrict__ ytab, int tiles_x, const uint8_t* __restrict__ src,
                                                      int spitch, size_t sframe, uint8_t* __restrict__ dst, int dpitch, size_t dframe,
                                                      int dw, int thin, int words) {
  constexpr int E = 4 * C;     // 16-bit sums (phase 1) / bytes (phase 2) of a work-item's 4 pixels
  constexpr int RW = 32 * C;   // words of an LDS row
  __shared__ uint32_t s_h[kRszSlots * RW];
  const int item = xcd_item(), f = xcd_frame(), tid = threadIdx.x;
  const int ty = item / tiles_x, tx = item - ty * tiles_x;
  const int g = tid & 15, r0 = tid >> 4;
  const int x0 = tx * kRszTileW + 4 * g;
  const ResizeRows* T = tiles + ty;
  const int dy0 = T->dy0, ndy = T->ndy, nsr = T->nsr;
  // everything the tables hold for this work-item is requested before the first tap
  const uint4* X4 = reinterpret_cast<const uint4*>(xtab + x0);
  const uint4 q0 = X4[0], q1 = X4[1];
  int srow[kRszPer];
  uint2 ry[kRszPer];
#pragma unroll
  for (int r = 0; r < kRszPer; ++r) {
    srow[r] = T->srow[imin(r0 + 16 * r, nsr - 1)];
    ry[r] = *reinterpret_cast<const uint2*>(ytab + dy0 + imin(r0 + 16 * r, ndy - 1));
  }
  const uint32_t win[4] = {q0.x, q0.z, q1.x, q1.z}, wt[4] = {q0.y, q0.w, q1.y, q1.w};
  const uint8_t* S = src + (size_t)f * sframe;
  if (x0 < dw) {
    uint32_t lo[kRszPer][4] = {}, hi[kRszPer][4] = {};
    if (!thin) {
#pragma unroll
      for (int r = 0; r < kRszPer; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint8_t* P = S + (size_t)srow[r] * spitch + (win[i] & 0xfffffu);
          lo[r][i] = load_u32_any(P);
          hi[r][i] = C > 1 ? load_u32_any(P + 4) : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < kRszPer; ++r) {
      if (r0 + 16 * r >= nsr) break;
      uint32_t pk[E / 2];
#pragma unroll
      for (int k = 0; k < E / 2; ++k) pk[k] = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t k0 = (win[i] >> 20) & 7u, k1 = (win[i] >> 24) & 15u, a0 = wt[i] & 0xffffu, a1 = wt[i] >> 16;
        uint32_t t0 = 0, t1 = 0;   // the left / right tap's channels, one per byte
        if (!thin) {
          const unsigned long long w = ((unsigned long long)hi[r][i] << 32) | lo[r][i];
          t0 = (uint32_t)(w >> (8 * k0));
          t1 = (uint32_t)(w >> (8 * k1));
        } else {
          const uint8_t* P = S + (size_t)srow[r] * spitch + (win[i] & 0xfffffu);
#pragma unroll
          for (int c = 0; c < C; ++c) { t0 |= (uint32_t)P[c] << (8 * c); t1 |= (uint32_t)P[k1 + c] << (8 * c); }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const uint32_t h = (((t0 >> (8 * c)) & 0xffu) * a0 + ((t1 >> (8 * c)) & 0xffu) * a1) >> 4;
          const int e = i * C + c;
          pk[e >> 1] |= h << (16 * (e & 1));
        }
      }
      uint2* H = reinterpret_cast<uint2*>(s_h + (r0 + 16 * r) * RW + g * (E / 2));
#pragma unroll
      for (int k = 0; k < E / 4; ++k) { uint2 v; v.x = pk[2 * k]; v.y = pk[2 * k + 1]; H[k] = v; }
    }
  }
  __syncthreads();
  if (x0 >= dw) return;
  const int n = imin(4, dw - x0);
#pragma unroll
  for (int r = 0; r < kRszPer; ++r) {
    const int row = r0 + 16 * r;
    if (row >= ndy) break;
    const uint2* H0 = reinterpret_cast<const uint2*>(s_h + (ry[r].x & 0xffu) * RW + g * (E / 2));
    const uint2* H1 = reinterpret_cast<const uint2*>(s_h + ((ry[r].x >> 8) & 0xffu) * RW + g * (E / 2));
    const int b0 = (int)(ry[r].y & 0xffffu), b1 = (int)(ry[r].y >> 16);
    uint32_t u0[E / 2], u1[E / 2];
#pragma unroll
    for (int k = 0; k < E / 4; ++k) {
      const uint2 a = H0[k], b = H1[k];
      u0[2 * k] = a.x; u0[2 * k + 1] = a.y; u1[2 * k] = b.x; u1[2 * k + 1] = b.y;
    }
    uint32_t out[C];
#pragma unroll
    for (int k = 0; k < C; ++k) out[k] = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int h0 = (int)((u0[e >> 1] >> (16 * (e & 1))) & 0xffffu), h1 = (int)((u1[e >> 1] >> (16 * (e & 1))) & 0xffffu);
      const int v = (((b0 * h0) >> 16) + ((b1 * h1) >> 16) + 2) >> 2;
      out[e >> 2] |= (uint32_t)(v & 0xff) << (8 * (e & 3));
    }
    uint8_t* D = dst + (size_t)f * dframe + (size_t)(dy0 + row) * dpitch + (size_t)x0 * C;
    if (n == 4 && words) {
#pragma unroll
      for (int k = 0; k < C; ++k) reinterpret_cast<uint32_t*>(D)[k] = out[k];
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (k < n * C) D[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace rgbl

using namespace rgbl;

struct rgbl_resizer {
  int device = 0;
  int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
  int tiles_x = 0, tiles_y = 0, area_fast = 0;
  bool thin[5] = {false, false, false, false, false};   // [C]: a source row is shorter than a pixel's window
  long long table_bytes = 0;
  bool xcd_map = true;              // RGBL_XCD_MAP=0, as for the extractor's pixel kernels
  uint8_t* d_tables = nullptr;      // one allocation: the x tables of C = 1, 3, 4 | the y table | the tile rows
  const ResizeX* d_xtab[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const ResizeY* d_ytab = nullptr;
  const ResizeRows* d_tiles = nullptr;
  // rgbl_resize (host pointers): one stream, grow-only source and destination staging
  hipStream_t stream = nullptr;
  void *d_src = nullptr, *d_dst = nullptr;
  size_t src_bytes = 0, dst_bytes = 0;
};

int rgbl_internal_resize_enqueue(rgbl_resizer* r, hipStream_t s, const uint8_t* d_src, int batch, int channels, int src_stride,
                                 size_t src_frame, uint8_t* d_dst, int dst_stride, size_t dst_frame) {
  const int words = ((reinterpret_cast<uintptr_t>(d_dst) | (uintptr_t)dst_stride | (uintptr_t)dst_frame) & 3u) == 0;
  const dim3 grid = xcd_grid(r->xcd_map, (unsigned)r->tiles_x * (unsigned)r->tiles_y, batch);
#define RGBL_RESIZE_LAUNCH(C)                                                                                                      \
  hipLaunchKernelGGL(k_resize_image<C>, grid, dim3(256), 0, s, r->d_tiles, r->d_xtab[C], r->d_ytab, r->tiles_x, d_src, src_stride, \
                     src_frame, d_dst, dst_stride, dst_frame, r->dst_w, (int)r->thin[C], words)
  if (channels == 1) RGBL_RESIZE_LAUNCH(1);
  else if (channels == 3) RGBL_RESIZE_LAUNCH(3);
  else RGBL_RESIZE_LAUNCH(4);
#undef RGBL_RESIZE_LAUNCH
  RGBL_HIP(hipGetLastError());
  return RGBL_OK;
}

int rgbl_internal_resizer_info(const rgbl_resizer* r, int* device, int* src_w, int* src_h, int* dst_w, int* dst_h) {
  if (!r) { set_error("null resizer"); return RGBL_ERR_INVALID; }
  *device = r->device; *src_w = r->src_w; *src_h = r->src_h; *dst_w = r->dst_w; *dst_h = r->dst_h;
  return RGBL_OK;
}

static int resize_check_layout(const rgbl_resizer* r, int batch, int channels, int src_stride, size_t src_frame, int dst_stride,
                               size_t dst_frame) {
  if ((channels != 1 && channels != 3 && channels != 4) || batch < 1 || src_stride < r->src_w * channels ||
      dst_stride < r->dst_w * channels ||
      (batch > 1 && (src_frame < (size_t)src_stride * r->src_h || dst_frame < (size_t)dst_stride * r->dst_h))) {
    set_error("resize: %d channels, batch %d, strides %d / %d are not a valid 8-bit batch for %dx%d -> %dx%d", channels, batch,
              src_stride, dst_stride, r->src_w, r->src_h, r->dst_w, r->dst_h);
    return RGBL_ERR_INVALID;
  }
  return RGBL_OK;
}

// the x table at C channels: windows in bytes, padded to whole tiles with copies of the last column
static void resize_x_entries(const std::vector<ResizeTab>& xt, int sw, int C, int padded, bool thin, ResizeX* out) {
  const int row_bytes = sw * C, wb = resize_window_bytes(C);
  for (int d = 0; d < padded; ++d) {
    const ResizeTab& t = xt[std::min(d, (int)xt.size() - 1)];
    const int base = t.sofs * C;
    const bool last = t.sofs >= sw - 1;               // the right tap lies outside the row; its weight is 0
    const int wofs = thin ? base : std::min(base, row_bytes - wb);
    const int k0 = base - wofs, k1 = last ? k0 : k0 + C;
    out[d].win = (uint32_t)wofs | ((uint32_t)k0 << 20) | ((uint32_t)k1 << 24);
    out[d].wt = (uint32_t)(uint16_t)t.a0 | ((uint32_t)(uint16_t)t.a1 << 16);
  }
}

extern "C" {

void rgbl_resizer_destroy(rgbl_resizer* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
  for (void* p : {(void*)r->d_tables, r->d_src, r->d_dst})
    if (p) (void)hipFree(p);
  delete r;
}

int rgbl_resizer_create(int device, int src_w, int src_h, int dst_w, int dst_h, rgbl_resizer** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1 || src_w > kResizeMaxSide || src_h > kResizeMaxSide ||
      dst_w > kResizeMaxSide || dst_h > kResizeMaxSide) {
    set_error("resizer: sides 1 .. %d (source %dx%d, destination %dx%d)", kResizeMaxSide, src_w, src_h, dst_w, dst_h);
    return RGBL_ERR_INVALID;
  }
  if (rgbl_device_count() <= device || device < 0) {
    set_error("no usable HIP device %d (this library has no CPU fallback)", device);
    return RGBL_ERR_NO_DEVICE;
  }
  RGBL_HIP(hipSetDevice(device));
  std::vector<ResizeTab> xt, yt;
  build_resize_tab(src_w, dst_w, true, xt);
  build_resize_tab(src_h, dst_h, false, yt);
  // tile rows: destination rows are taken while the tile has room for them and for the source rows they add
  std::vector<ResizeRows> rows;
  std::vector<ResizeY> ytab(dst_h);
  for (int dy = 0; dy < dst_h;) {
    ResizeRows T;
    memset(&T, 0, sizeof(T));
    T.dy0 = dy;
    for (; dy < dst_h && T.ndy < kRszRows; ++dy, ++T.ndy) {
      const int need[2] = {std::min(std::max(yt[dy].sofs, 0), src_h - 1), std::min(std::max(yt[dy].sofs + 1, 0), src_h - 1)};
      int slot[2], nsr = T.nsr;
      for (int k = 0; k < 2; ++k) {
        slot[k] = (int)(std::find(T.srow, T.srow + nsr, need[k]) - T.srow);
        if (slot[k] == nsr && nsr < kRszSlots) T.srow[nsr++] = need[k];
        else if (slot[k] == nsr) slot[k] = -1;
      }
      if (slot[0] < 0 || slot[1] < 0) break;   // no room: the row opens the next tile (srow entries beyond nsr are never read)
      T.nsr = nsr;
      ytab[dy].slots = (uint32_t)slot[0] | ((uint32_t)slot[1] << 8);
      ytab[dy].wt = (uint32_t)(uint16_t)yt[dy].a0 | ((uint32_t)(uint16_t)yt[dy].a1 << 16);
    }
    rows.push_back(T);
  }
  rgbl_resizer* r = new rgbl_resizer;
  r->device = device; r->src_w = src_w; r->src_h = src_h; r->dst_w = dst_w; r->dst_h = dst_h;
  r->tiles_x = (dst_w + kRszTileW - 1) / kRszTileW; r->tiles_y = (int)rows.size();
  // resize.cpp: INTER_LINEAR && is_area_fast && iscale_x == 2 && iscale_y == 2 -> INTER_AREA
  const double scale_x = 1.0 / ((double)dst_w / src_w), scale_y = 1.0 / ((double)dst_h / src_h);
  r->area_fast = fabs(scale_x - 2.0) < DBL_EPSILON && fabs(scale_y - 2.0) < DBL_EPSILON;
  if (const char* v = getenv("RGBL_XCD_MAP")) r->xcd_map = v[0] != '0';
  const int padded = r->tiles_x * kRszTileW;
  const size_t x_bytes = sizeof(ResizeX) * padded, y_bytes = sizeof(ResizeY) * dst_h, t_bytes = sizeof(ResizeRows) * rows.size();
  std::vector<uint8_t> host(3 * x_bytes + y_bytes + t_bytes);
  int k = 0;
  for (int c : {1, 3, 4}) {
    r->thin[c] = src_w * c < resize_window_bytes(c);
    resize_x_entries(xt, src_w, c, padded, r->thin[c], reinterpret_cast<ResizeX*>(host.data() + x_bytes * k++));
  }
  memcpy(host.data() + 3 * x_bytes, ytab.data(), y_bytes);
  memcpy(host.data() + 3 * x_bytes + y_bytes, rows.data(), t_bytes);
  r->table_bytes = (long long)host.size();
  const bool ok = rgbl::device_alloc(&r->d_tables, host.size()) == hipSuccess && hipStreamCreate(&r->stream) == hipSuccess &&
                  hipMemcpy(r->d_tables, host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    set_error("resizer: device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    rgbl_resizer_destroy(r);
    return RGBL_ERR_HIP;
  }
  k = 0;
  for (int c : {1, 3, 4}) r->d_xtab[c] = reinterpret_cast<const ResizeX*>(r->d_tables + x_bytes * k++);
  r->d_ytab = reinterpret_cast<const ResizeY*>(r->d_tables + 3 * x_bytes);
  r->d_tiles = reinterpret_cast<const ResizeRows*>(r->d_tables + 3 * x_bytes + y_bytes);
  *out = r;
  return RGBL_OK;
}

int rgbl_resizer_info(const rgbl_resizer* r, int* src_w, int* src_h, int* dst_w, int* dst_h, int* area_fast, long long* table_bytes) {
  if (!r) { set_error("null resizer"); return RGBL_ERR_INVALID; }
  if (src_w) *src_w = r->src_w;
  if (src_h) *src_h = r->src_h;
  if (dst_w) *dst_w = r->dst_w;
  if (dst_h) *dst_h = r->dst_h;
  if (area_fast) *area_fast = r->area_fast;
  if (table_bytes) *table_bytes = r->table_bytes;
  return RGBL_OK;
}

int rgbl_resize_batch_device(rgbl_resizer* r, rgbl_extractor* e, const uint8_t* d_src, int batch, int channels, int src_stride,
                             size_t src_frame_stride, uint8_t* d_dst, int dst_stride, size_t dst_frame_stride) {
  if (!r || !e || !d_src || !d_dst) { set_error("null argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(resize_check_layout(r, batch, channels, src_stride, src_frame_stride, dst_stride, dst_frame_stride));
  int w = 0, h = 0, max_batch = 0, device = 0;
  int* d_err = nullptr;
  RGBL_TRY(rgbl_internal_extractor_info(e, &w, &h, &max_batch, &device, &d_err));
  if (batch > max_batch) { set_error("resize: batch %d exceeds the extractor's max_batch %d", batch, max_batch); return RGBL_ERR_INVALID; }
  if (device != r->device) { set_error("resizer and extractor live on different devices"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(r->device));
  return rgbl_internal_resize_enqueue(r, (hipStream_t)rgbl_extractor_stream(e), d_src, batch, channels, src_stride, src_frame_stride,
                                      d_dst, dst_stride, dst_frame_stride);
}

int rgbl_resize(rgbl_resizer* r, const uint8_t* src, int channels, int src_stride, uint8_t* dst, int dst_stride) {
  if (!r || !src || !dst) { set_error("null argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(resize_check_layout(r, 1, channels, src_stride, 0, dst_stride, 0));
  RGBL_HIP(hipSetDevice(r->device));
  hipStream_t s = r->stream;
  StreamDrain drain(s);
  // rows packed to a multiple of 4 bytes on the device; a host image with that very stride travels as one linear copy
  const int sp = (r->src_w * channels + 3) & ~3, dp = (r->dst_w * channels + 3) & ~3;
  RGBL_TRY(grow_staging(&r->d_src, &r->src_bytes, (size_t)sp * r->src_h + 16));
  RGBL_TRY(grow_staging(&r->d_dst, &r->dst_bytes, (size_t)dp * r->dst_h + 16));
  uint8_t *ds = (uint8_t*)r->d_src, *dd = (uint8_t*)r->d_dst;
  if (src_stride == sp) RGBL_HIP(hipMemcpyAsync(ds, src, (size_t)(r->src_h - 1) * sp + (size_t)r->src_w * channels, hipMemcpyHostToDevice, s));
  else RGBL_HIP(hipMemcpy2DAsync(ds, sp, src, src_stride, (size_t)r->src_w * channels, r->src_h, hipMemcpyHostToDevice, s));
  RGBL_TRY(rgbl_internal_resize_enqueue(r, s, ds, 1, channels, sp, 0, dd, dp, 0));
  if (dst_stride == dp) RGBL_HIP(hipMemcpyAsync(dst, dd, (size_t)(r->dst_h - 1) * dp + (size_t)r->dst_w * channels, hipMemcpyDeviceToHost, s));
  else RGBL_HIP(hipMemcpy2DAsync(dst, dst_stride, dd, dp, (size_t)r->dst_w * channels, r->dst_h, hipMemcpyDeviceToHost, s));
  RGBL_HIP(hipStreamSynchronize(s));
  return RGBL_OK;
}

}  // extern "C"
