// rectify.hip — the stereo rectification in front of the extractor: cv::remap(src, dst, M1, M2, cv::INTER_LINEAR) of
// System::TrackStereo (src/System.cc:260-268) on 8-bit images with 1, 3 or 4 interleaved channels, two CV_32FC1 maps,
// BORDER_CONSTANT 0.  Restated from OpenCV 4.x imgproc/src/remap.cpp (parity vs the restatement, unpinned):
//   sx = cvRound(map_x * 32) (fp32 product, half-to-even, NaN / |v| >= 2^31 -> INT32_MIN), ix = sat_short(sx >> 5), fx = sx & 31
//   dst = (sum of the four taps x their 10-bit weights + 512) >> 10, a tap outside the image is 0
// (OpenCV's 15-bit table holds 32 x these weights, so (sum + 2^14) >> 15 is the same number).
//
// The float maps are turned into fixed point ONCE, on the host, when the handle is created.  The destination is cut into
// tiles of 64 x 32 pixels; every tile gets a record with the bounding box of the source pixels its taps touch:
//   k_remap_linear  "staged" tiles: the box fits the LDS budget.  The workgroup copies the box into LDS (32-bit loads, what
//                   lies outside the image is written as 0), then every work-item produces 4 consecutive pixels from one
//                   16-byte load of 4-byte map entries (box-relative ix, iy: 8 bits each, fx, fy: 5 bits each) - no
//                   per-tap bounds test.
//   k_remap_gather  "direct" tiles (random maps, strong minification): 8-byte entries (sx, sy), per-tap bounds tests,
//                   byte loads from global memory at addresses clamped into the image.
// Both kinds keep their entries tile by tile (2048 per tile), so a workgroup's map traffic is one contiguous block.  The map
// entries are requested before the box is staged, and the words of the box four at a time before the first of them is written
// to LDS (worth 4 - 9 % when measured; DESIGN 9 has the kernels' share of the copy ceiling).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.h"

namespace rgbl {

constexpr int kRemapTileW = 64, kRemapTileH = 32;      // 256 work-items x 4 pixels x kRemapRows rows
constexpr int kRemapRows = kRemapTileH / 16;           // work-item (tid & 15, tid >> 4) owns the rows (tid >> 4) + 16 r
constexpr int kRemapTilePx = kRemapTileW * kRemapTileH;
constexpr int kRemapLdsWords = 6144;                   // a box may take 24 KiB with 4 channels; a launch asks for what ITS boxes need (lds_words)
constexpr uint32_t kRemapOutside = 0x80000000u;        // staged entry: all four taps outside the image -> 0
constexpr int kRemapMaxSide = 16384;                   // so that a saturated ix / iy (+-32768) is always outside

// One destination tile.  (bx0, by0) .. + (bw, bh): the source pixels of its taps, inside [-1, src_w] x [-1, src_h].
struct RemapTile { int16_t bx0, by0; uint16_t bw, bh, tx, ty; uint32_t pad; };
struct alignas(8) RemapFixed { int32_t x, y; };      // a direct tile's entry: cvRound(map * 32) of both axes

// words of LDS a box takes at C channels (the box may start at any byte of a word; + 1 word per row: taps are read as words)
static inline int remap_box_words(int bw, int bh, int C) { return ((3 + bw * C + 3) / 4 + 1) * bh; }
// the budget is tested for 4 channels, so a tile's path does not depend on the image type
static inline bool remap_box_fits(int bw, int bh) {
  return bw <= 257 && bh <= 257 && remap_box_words(bw, bh, 4) <= kRemapLdsWords;
}

template <int C>
__device__ __forceinline__ void remap_store4(uint8_t* D, const uint32_t (&px)[4][4], int n, bool words) {
  // px[i][c]: pixel i, channel c
  if (n == 4 && words) {
    uint32_t* W = reinterpret_cast<uint32_t*>(D);
    if (C == 1) W[0] = px[0][0] | (px[1][0] << 8) | (px[2][0] << 16) | (px[3][0] << 24);
    if (C == 3) {
      W[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
      W[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
      W[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    }
    if (C == 4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) W[i] = px[i][0] | (px[i][1] << 8) | (px[i][2] << 16) | (px[i][3] << 24);
    }
    return;
  }
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < C; ++c) D[i * C + c] = (uint8_t)px[i][c];
}

// grid = xcd_grid(staged tiles, B) (common.h), block = 256, dynamic LDS = rgbl_rectifier::lds_words[C] words.
// words: destination base and strides are multiples of 4.
template <int C>
__global__ __launch_bounds__(256) void k_remap_linear(const RemapTile* __restrict__ tiles, const uint32_t* __restrict__ map4,
                                                      const uint8_t* __restrict__ src, int spitch, size_t sframe, int sw, int sh,
                                                      uint8_t* __restrict__ dst, int dpitch, size_t dframe, int dw, int dh, int words) {
  RGBL_DYN_SHARED(uint32_t, s_box);   // the largest box of the rectifier's staged tiles at C channels
  const int t = xcd_item(), f = xcd_frame(), tid = threadIdx.x;
  const RemapTile T = tiles[t];
  const int bx0 = T.bx0, by0 = T.by0, bh = T.bh;
  const int bxb0 = (bx0 * C) & ~3;                           // first byte column of the box's words (-4 for a box that starts at -1)
  const int xoff = bx0 * C - bxb0;                           // 0 .. 3
  const int pw = (xoff + (int)T.bw * C + 3) / 4 + 1;         // words per box row; + 1: a tap pair is read as whole words
  const int row_bytes = sw * C;
  const uint8_t* S = src + (size_t)f * sframe;
  // the map entries do not depend on the box: on their way while it is staged
  uint4 e4[kRemapRows];
#pragma unroll
  for (int r = 0; r < kRemapRows; ++r) e4[r] = *reinterpret_cast<const uint4*>(map4 + (size_t)t * kRemapTilePx + (size_t)(r * 256 + tid) * 4);
  auto fetch = [&](int i) -> uint32_t {
    const int r = (int)((uint32_t)i / (uint32_t)pw), w = i - r * pw;
    const int sr = by0 + r, b0 = bxb0 + 4 * w;
    uint32_t v = 0;
    if (sr >= 0 && sr < sh) {
      const uint8_t* R = S + (size_t)sr * spitch;
      if (b0 >= 0 && b0 + 4 <= row_bytes) v = load_u32_any(R + b0);
      else
        for (int k = 0; k < 4; ++k)
          if (b0 + k >= 0 && b0 + k < row_bytes) v |= (uint32_t)R[b0 + k] << (8 * k);
    }
    return v;
  };
  const int n_words = pw * bh;
  for (int base = tid; base < n_words; base += 1024) {
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = base + 256 * k < n_words ? fetch(base + 256 * k) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (base + 256 * k < n_words) s_box[base + 256 * k] = v[k];
  }
  __syncthreads();
  const int x0 = T.tx * kRemapTileW + (tid & 15) * 4;
  if (x0 >= dw) return;
  const uint8_t* B = reinterpret_cast<const uint8_t*>(s_box);
#pragma unroll
  for (int rr = 0; rr < kRemapRows; ++rr) {
    const int y = T.ty * kRemapTileH + rr * 16 + (tid >> 4);
    if (y >= dh) break;
    const uint32_t ent[4] = {e4[rr].x, e4[rr].y, e4[rr].z, e4[rr].w};
    uint32_t px[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t e = ent[i];
      const int ix = e & 0xff, iy = (e >> 8) & 0xff;
      const uint32_t fx = (e >> 16) & 31, fy = (e >> 21) & 31;
      const uint8_t* P0 = B + (size_t)(iy * pw) * 4 + xoff + ix * C;
      const uint8_t* P1 = P0 + (size_t)pw * 4;
      // both taps of a row: 2 * C bytes, read as one or two (unaligned) LDS words
      uint32_t a0 = load_u32_any(P0), b0 = load_u32_any(P1), a1 = 0, b1 = 0;
      if (C > 1) { a1 = load_u32_any(P0 + 4); b1 = load_u32_any(P1 + 4); }
      const uint32_t keep = (e & kRemapOutside) ? 0u : 0xffffffffu;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        // byte c of the left tap, byte C + c of the right one
        const int l = c, r = C + c;
        const uint32_t t00 = ((l < 4 ? a0 >> (8 * l) : a1 >> (8 * (l - 4))) & 0xffu), t01 = ((r < 4 ? a0 >> (8 * r) : a1 >> (8 * (r - 4))) & 0xffu);
        const uint32_t t10 = ((l < 4 ? b0 >> (8 * l) : b1 >> (8 * (l - 4))) & 0xffu), t11 = ((r < 4 ? b0 >> (8 * r) : b1 >> (8 * (r - 4))) & 0xffu);
        const uint32_t h0 = t00 * (32u - fx) + t01 * fx, h1 = t10 * (32u - fx) + t11 * fx;   // exact: integer arithmetic distributes
        px[i][c] = ((h0 * (32u - fy) + h1 * fy + 512u) >> 10) & keep;
      }
    }
    remap_store4<C>(dst + (size_t)f * dframe + (size_t)y * dpitch + (size_t)x0 * C, px, imin(4, dw - x0), words != 0);
  }
}

// grid = xcd_grid(direct tiles, B), block = 256.  Every address is built from coordinates clamped into the image; the
// bounds test only selects between the loaded byte and 0.
template <int C>
__global__ __launch_bounds__(256) void k_remap_gather(const RemapTile* __restrict__ tiles, const RemapFixed* __restrict__ map8,
                                                      const uint8_t* __restrict__ src, int spitch, size_t sframe, int sw, int sh,
                                                      uint8_t* __restrict__ dst, int dpitch, size_t dframe, int dw, int dh, int words) {
  const int t = xcd_item(), f = xcd_frame(), tid = threadIdx.x;
  const RemapTile T = tiles[t];
  const int x0 = T.tx * kRemapTileW + (tid & 15) * 4;
  if (x0 >= dw) return;
  const uint8_t* S = src + (size_t)f * sframe;
  for (int rr = 0; rr < kRemapRows; ++rr) {
    const int y = T.ty * kRemapTileH + rr * 16 + (tid >> 4);
    if (y >= dh) break;
    const RemapFixed* M = map8 + (size_t)t * kRemapTilePx + (size_t)(rr * 256 + tid) * 4;
    uint32_t px[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const RemapFixed m = M[i];
      const int ix = imin(imax(m.x >> 5, -32768), 32767), iy = imin(imax(m.y >> 5, -32768), 32767);
      const uint32_t fx = (uint32_t)m.x & 31u, fy = (uint32_t)m.y & 31u;
      const bool inx0 = ix >= 0 && ix < sw, inx1 = ix + 1 >= 0 && ix + 1 < sw, iny0 = iy >= 0 && iy < sh, iny1 = iy + 1 >= 0 && iy + 1 < sh;
      const int qx0 = imin(imax(ix, 0), sw - 1), qx1 = imin(imax(ix + 1, 0), sw - 1);
      const int qy0 = imin(imax(iy, 0), sh - 1), qy1 = imin(imax(iy + 1, 0), sh - 1);
      const uint8_t* R0 = S + (size_t)qy0 * spitch;
      const uint8_t* R1 = S + (size_t)qy1 * spitch;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t v00 = R0[qx0 * C + c], v01 = R0[qx1 * C + c], v10 = R1[qx0 * C + c], v11 = R1[qx1 * C + c];
        const uint32_t t00 = (inx0 && iny0) ? v00 : 0u, t01 = (inx1 && iny0) ? v01 : 0u;
        const uint32_t t10 = (inx0 && iny1) ? v10 : 0u, t11 = (inx1 && iny1) ? v11 : 0u;
        const uint32_t h0 = t00 * (32u - fx) + t01 * fx, h1 = t10 * (32u - fx) + t11 * fx;
        px[i][c] = (h0 * (32u - fy) + h1 * fy + 512u) >> 10;
      }
    }
    remap_store4<C>(dst + (size_t)f * dframe + (size_t)y * dpitch + (size_t)x0 * C, px, imin(4, dw - x0), words != 0);
  }
}

// cvRound(v * 32) as x86's cvtss2si gives it (OpenCV's cvRound): half-to-even, NaN and |v| >= 2^31 -> INT32_MIN
static inline int32_t remap_fixed(float m) {
  const float v = m * 32.0f;
  if (!(fabsf(v) < 2147483648.0f)) return INT32_MIN;
  return (int32_t)lrintf(v);
}

}  // namespace rgbl

using namespace rgbl;

struct rgbl_rectifier {
  int device = 0;
  int src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
  int n_staged = 0, n_direct = 0;
  int lds_words[5] = {0, 0, 0, 0, 0};   // [C]: the largest staged box at C channels = dynamic LDS of k_remap_linear<C>
  long long map_bytes = 0;
  bool xcd_map = true;              // RGBL_XCD_MAP=0, as for the extractor's pixel kernels
  RemapTile* d_tiles = nullptr;     // staged tiles first, then the direct ones
  uint32_t* d_map4 = nullptr;       // [n_staged][kRemapTilePx]
  RemapFixed* d_map8 = nullptr;           // [n_direct][kRemapTilePx]
  // rgbl_remap (host pointers): one stream, source and destination staging for up to 4 channels, allocated at creation
  hipStream_t stream = nullptr;
  uint8_t *d_src = nullptr, *d_dst = nullptr;
};

int rgbl_internal_remap_enqueue(rgbl_rectifier* r, hipStream_t s, const uint8_t* d_src, int batch, int channels, int src_stride,
                                size_t src_frame, uint8_t* d_dst, int dst_stride, size_t dst_frame) {
  const int words = ((reinterpret_cast<uintptr_t>(d_dst) | (uintptr_t)dst_stride | (uintptr_t)dst_frame) & 3u) == 0;
#define RGBL_REMAP_LAUNCH(C)                                                                                                       \
  do {                                                                                                                             \
    if (r->n_staged)                                                                                                               \
      hipLaunchKernelGGL(k_remap_linear<C>, xcd_grid(r->xcd_map, r->n_staged, batch), dim3(256), sizeof(uint32_t) * r->lds_words[C], s, r->d_tiles, r->d_map4, d_src, \
                         src_stride, src_frame, r->src_w, r->src_h, d_dst, dst_stride, dst_frame, r->dst_w, r->dst_h, words);      \
    if (r->n_direct)                                                                                                               \
      hipLaunchKernelGGL(k_remap_gather<C>, xcd_grid(r->xcd_map, r->n_direct, batch), dim3(256), 0, s, r->d_tiles + r->n_staged,   \
                         r->d_map8, d_src, src_stride, src_frame, r->src_w, r->src_h, d_dst, dst_stride, dst_frame, r->dst_w,      \
                         r->dst_h, words);                                                                                         \
  } while (0)
  if (channels == 1) RGBL_REMAP_LAUNCH(1);
  else if (channels == 3) RGBL_REMAP_LAUNCH(3);
  else RGBL_REMAP_LAUNCH(4);
#undef RGBL_REMAP_LAUNCH
  RGBL_HIP(hipGetLastError());
  return RGBL_OK;
}

int rgbl_internal_rectifier_info(const rgbl_rectifier* r, int* device, int* src_w, int* src_h, int* dst_w, int* dst_h) {
  if (!r) { set_error("null rectifier"); return RGBL_ERR_INVALID; }
  *device = r->device; *src_w = r->src_w; *src_h = r->src_h; *dst_w = r->dst_w; *dst_h = r->dst_h;
  return RGBL_OK;
}

static int remap_check_layout(const rgbl_rectifier* r, int batch, int channels, int src_stride, size_t src_frame, int dst_stride,
                              size_t dst_frame) {
  if ((channels != 1 && channels != 3 && channels != 4) || batch < 1 || src_stride < r->src_w * channels ||
      dst_stride < r->dst_w * channels ||
      (batch > 1 && (src_frame < (size_t)src_stride * r->src_h || dst_frame < (size_t)dst_stride * r->dst_h))) {
    set_error("remap: %d channels, batch %d, strides %d / %d are not a valid 8-bit batch for %dx%d -> %dx%d", channels, batch,
              src_stride, dst_stride, r->src_w, r->src_h, r->dst_w, r->dst_h);
    return RGBL_ERR_INVALID;
  }
  return RGBL_OK;
}

extern "C" {

void rgbl_rectifier_destroy(rgbl_rectifier* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) { (void)hipStreamSynchronize(r->stream); (void)hipStreamDestroy(r->stream); }
  for (void* p : {(void*)r->d_tiles, (void*)r->d_map4, (void*)r->d_map8, (void*)r->d_src, (void*)r->d_dst})
    if (p) (void)hipFree(p);
  delete r;
}

int rgbl_rectifier_create(int device, int src_w, int src_h, int dst_w, int dst_h, const float* map_x, const float* map_y,
                          int map_stride_floats, rgbl_rectifier** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (!map_x || !map_y || src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1 || src_w > kRemapMaxSide || src_h > kRemapMaxSide ||
      dst_w > kRemapMaxSide || dst_h > kRemapMaxSide || map_stride_floats < dst_w) {
    set_error("rectifier: two float maps of the destination's size, sides 1 .. %d (source %dx%d, destination %dx%d, map stride %d)",
              kRemapMaxSide, src_w, src_h, dst_w, dst_h, map_stride_floats);
    return RGBL_ERR_INVALID;
  }
  if (rgbl_device_count() <= device || device < 0) {
    set_error("no usable HIP device %d (this library has no CPU fallback)", device);
    return RGBL_ERR_NO_DEVICE;
  }
  RGBL_HIP(hipSetDevice(device));
  const int tiles_x = (dst_w + kRemapTileW - 1) / kRemapTileW, tiles_y = (dst_h + kRemapTileH - 1) / kRemapTileH;
  const int n_tiles = tiles_x * tiles_y;
  // pass 1: fixed point (sx, sy) of every destination pixel, tile by tile; the box of every tile
  std::vector<RemapFixed> fixed((size_t)n_tiles * kRemapTilePx);
  std::vector<RemapTile> rec(n_tiles);
  std::vector<uint8_t> staged(n_tiles);
  int n_staged = 0;
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      const int t = ty * tiles_x + tx;
      RemapFixed* F = &fixed[(size_t)t * kRemapTilePx];
      int x_lo = INT32_MAX, x_hi = INT32_MIN, y_lo = INT32_MAX, y_hi = INT32_MIN;
      for (int j = 0; j < kRemapTileH; ++j)
        for (int i = 0; i < kRemapTileW; ++i) {
          const int x = tx * kRemapTileW + i, y = ty * kRemapTileH + j;
          RemapFixed m;
          m.x = m.y = INT32_MIN;   // beyond the destination: never stored
          if (x < dst_w && y < dst_h) {
            m.x = remap_fixed(map_x[(size_t)y * map_stride_floats + x]);
            m.y = remap_fixed(map_y[(size_t)y * map_stride_floats + x]);
            const int ix = std::min(std::max(m.x >> 5, -32768), 32767), iy = std::min(std::max(m.y >> 5, -32768), 32767);
            if (ix >= -1 && ix < src_w && iy >= -1 && iy < src_h) {   // at least one tap inside
              x_lo = std::min(x_lo, ix); x_hi = std::max(x_hi, ix + 1);
              y_lo = std::min(y_lo, iy); y_hi = std::max(y_hi, iy + 1);
            }
          }
          F[j * kRemapTileW + i] = m;
        }
      RemapTile& T = rec[t];
      memset(&T, 0, sizeof(T));
      T.tx = (uint16_t)tx; T.ty = (uint16_t)ty;
      if (x_lo > x_hi) { x_lo = 0; x_hi = 1; y_lo = 0; y_hi = 1; }   // nothing inside: any box, every entry is flagged
      T.bx0 = (int16_t)x_lo; T.by0 = (int16_t)y_lo;
      const int bw = x_hi - x_lo + 1, bh = y_hi - y_lo + 1;
      staged[t] = remap_box_fits(bw, bh);
      T.bw = (uint16_t)std::min(bw, 65535); T.bh = (uint16_t)std::min(bh, 65535);
      n_staged += staged[t];
    }
  int lds_words[5] = {0, 0, 0, 0, 0};
  for (int t = 0; t < n_tiles; ++t)
    if (staged[t])
      for (int c : {1, 3, 4}) lds_words[c] = std::max(lds_words[c], remap_box_words(rec[t].bw, rec[t].bh, c));
  const int n_direct = n_tiles - n_staged;
  // pass 2: the two entry arrays and the tile list, staged tiles first
  std::vector<RemapTile> order(n_tiles);
  std::vector<uint32_t> map4((size_t)std::max(n_staged, 1) * kRemapTilePx);
  std::vector<RemapFixed> map8((size_t)std::max(n_direct, 1) * kRemapTilePx);
  int ks = 0, kd = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const RemapFixed* F = &fixed[(size_t)t * kRemapTilePx];
    if (!staged[t]) {
      order[n_staged + kd] = rec[t];
      memcpy(&map8[(size_t)kd * kRemapTilePx], F, sizeof(RemapFixed) * kRemapTilePx);
      ++kd;
      continue;
    }
    order[ks] = rec[t];
    uint32_t* M = &map4[(size_t)ks * kRemapTilePx];
    ++ks;
    for (int k = 0; k < kRemapTilePx; ++k) {
      const int ix = std::min(std::max(F[k].x >> 5, -32768), 32767), iy = std::min(std::max(F[k].y >> 5, -32768), 32767);
      if (ix >= -1 && ix < src_w && iy >= -1 && iy < src_h)
        M[k] = (uint32_t)(ix - rec[t].bx0) | ((uint32_t)(iy - rec[t].by0) << 8) | (((uint32_t)F[k].x & 31u) << 16) | (((uint32_t)F[k].y & 31u) << 21);
      else
        M[k] = kRemapOutside;
    }
  }
  rgbl_rectifier* r = new rgbl_rectifier;
  r->device = device; r->src_w = src_w; r->src_h = src_h; r->dst_w = dst_w; r->dst_h = dst_h;
  r->n_staged = n_staged; r->n_direct = n_direct;
  memcpy(r->lds_words, lds_words, sizeof(lds_words));
  if (const char* v = getenv("RGBL_XCD_MAP")) r->xcd_map = v[0] != '0';
  const size_t tile_bytes = sizeof(RemapTile) * n_tiles, m4 = sizeof(uint32_t) * map4.size(), m8 = sizeof(RemapFixed) * map8.size();
  r->map_bytes = (long long)(tile_bytes + (n_staged ? m4 : 0) + (n_direct ? m8 : 0));
  const size_t src_bytes = (size_t)src_w * 4 * src_h + 16, dst_bytes = (size_t)dst_w * 4 * dst_h + 16;
  const bool ok = rgbl::device_alloc(&r->d_tiles, tile_bytes) == hipSuccess && rgbl::device_alloc(&r->d_map4, m4) == hipSuccess &&
                  rgbl::device_alloc(&r->d_map8, m8) == hipSuccess && rgbl::device_alloc(&r->d_src, src_bytes) == hipSuccess &&
                  rgbl::device_alloc(&r->d_dst, dst_bytes) == hipSuccess && hipStreamCreate(&r->stream) == hipSuccess &&
                  hipMemcpy(r->d_tiles, order.data(), tile_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(r->d_map4, map4.data(), m4, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(r->d_map8, map8.data(), m8, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    set_error("rectifier: device allocation / upload failed: %s", hipGetErrorString(hipGetLastError()));
    rgbl_rectifier_destroy(r);
    return RGBL_ERR_HIP;
  }
  *out = r;
  return RGBL_OK;
}

int rgbl_rectifier_info(const rgbl_rectifier* r, int* src_w, int* src_h, int* dst_w, int* dst_h, int* staged_tiles,
                        int* direct_tiles, long long* map_bytes) {
  if (!r) { set_error("null rectifier"); return RGBL_ERR_INVALID; }
  if (src_w) *src_w = r->src_w;
  if (src_h) *src_h = r->src_h;
  if (dst_w) *dst_w = r->dst_w;
  if (dst_h) *dst_h = r->dst_h;
  if (staged_tiles) *staged_tiles = r->n_staged;
  if (direct_tiles) *direct_tiles = r->n_direct;
  if (map_bytes) *map_bytes = r->map_bytes;
  return RGBL_OK;
}

int rgbl_remap_batch_device(rgbl_rectifier* r, rgbl_extractor* e, const uint8_t* d_src, int batch, int channels, int src_stride,
                            size_t src_frame_stride, uint8_t* d_dst, int dst_stride, size_t dst_frame_stride) {
  if (!r || !e || !d_src || !d_dst) { set_error("null argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(remap_check_layout(r, batch, channels, src_stride, src_frame_stride, dst_stride, dst_frame_stride));
  int w = 0, h = 0, max_batch = 0, device = 0;
  int* d_err = nullptr;
  RGBL_TRY(rgbl_internal_extractor_info(e, &w, &h, &max_batch, &device, &d_err));
  if (device != r->device) { set_error("rectifier and extractor live on different devices"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(r->device));
  return rgbl_internal_remap_enqueue(r, (hipStream_t)rgbl_extractor_stream(e), d_src, batch, channels, src_stride, src_frame_stride,
                                     d_dst, dst_stride, dst_frame_stride);
}

int rgbl_remap(rgbl_rectifier* r, const uint8_t* src, int channels, int src_stride, uint8_t* dst, int dst_stride) {
  if (!r || !src || !dst) { set_error("null argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(remap_check_layout(r, 1, channels, src_stride, 0, dst_stride, 0));
  RGBL_HIP(hipSetDevice(r->device));
  hipStream_t s = r->stream;
  StreamDrain drain(s);
  // rows packed to a multiple of 4 bytes on the device; a host image with that very stride travels as one linear copy
  const int sp = (r->src_w * channels + 3) & ~3, dp = (r->dst_w * channels + 3) & ~3;
  if (src_stride == sp) RGBL_HIP(hipMemcpyAsync(r->d_src, src, (size_t)(r->src_h - 1) * sp + (size_t)r->src_w * channels, hipMemcpyHostToDevice, s));
  else RGBL_HIP(hipMemcpy2DAsync(r->d_src, sp, src, src_stride, (size_t)r->src_w * channels, r->src_h, hipMemcpyHostToDevice, s));
  RGBL_TRY(rgbl_internal_remap_enqueue(r, s, r->d_src, 1, channels, sp, 0, r->d_dst, dp, 0));
  if (dst_stride == dp) RGBL_HIP(hipMemcpyAsync(dst, r->d_dst, (size_t)(r->dst_h - 1) * dp + (size_t)r->dst_w * channels, hipMemcpyDeviceToHost, s));
  else RGBL_HIP(hipMemcpy2DAsync(dst, dst_stride, r->d_dst, dp, (size_t)r->dst_w * channels, r->dst_h, hipMemcpyDeviceToHost, s));
  RGBL_HIP(hipStreamSynchronize(s));
  return RGBL_OK;
}

}  // extern "C"
