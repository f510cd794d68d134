// matcher.hip — 256-bit Hamming matching: brute force best/second-best and SearchForTriangulation.
//
// Replaces ORB_SLAM3::ORBmatcher::DescriptorDistance (/root/reference/src/ORBmatcher.cc:2058-2074),
// ORBmatcher::SearchForTriangulation (:907-1146) incl. ComputeThreeMaxima (:2012-2053) and the pinhole
// epipolar test (/root/reference/src/CameraModels/Pinhole.cpp:107-129).
//
// Kernels:
//   k_hamming_bf          one query descriptor per lane (4 x u64 in VGPRs); the train descriptors are read
//                         through wave-uniform addresses (scalar loads, broadcast to the 64 lanes), XOR +
//                         v_bcnt popcount, running best / second-best with the reference's strict '<'.
//   k_search_triangulation one workgroup per BoW node shared by both key-frames, both buckets staged in LDS, one
//                         query feature per wave, the candidates over its lanes (ties -> later candidate wins, as
//                         in the reference) with the eligibility masks and epipolar test.
//
// What else lives here, each under its own heading: the matrix-core forms of the scan (k_hamming_mfma, k_hamming_fp4), the
// projection, fuse, local-map and initialisation searches (k_proj_*, k_fuse_search, k_local_*, k_init_*), SearchByBoW and the
// vocabulary descent (k_search_by_bow*, k_bow_descend), CreateNewMapPoints (k_new_points), the frustum test, the map-point
// pool and its refresh (k_frustum, k_map_points_scatter, k_map_refresh_*), and the handles: matcher, matcher pool, resident
// frames, map points, vocabulary.  The scaffold of a host-pointer call is csrc/matcher_call.h; the geometry solvers that
// share it are csrc/optimize.hip (PoseOptimization, OptimizeSim3), csrc/ransac.hip (Sim3Solver, MLPnPsolver,
// TwoViewReconstruction) and csrc/lba.hip (LocalBundleAdjustment).
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <functional>
#include <mutex>
#include <utility>
#include <vector>

#include "common.h"
#include "matcher_call.h"
#include "frustum_math.h"
#include "logf_glibc.h"
#include "newpoint_math.h"

namespace rgbl {

__device__ __forceinline__ int hamming256(const unsigned long long q[4], const unsigned long long* __restrict__ t) {
  // one accumulating chain of eight 32-bit popcounts (v_bcnt_u32_b32 adds its second operand for free); four 64-bit
  // popcounts cost the same eight v_bcnt plus two adds for the partial sums
  // (written as inline assembly: the compiler re-balances a chain of ctpop + add into a tree with three v_add3 per distance)
  uint32_t acc = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long x = q[k] ^ t[k];
#ifdef RGBL_EMU
    acc += (uint32_t)__builtin_popcountll(x);
#else
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(acc) : "v"((uint32_t)x), "v"(acc));
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(acc) : "v"((uint32_t)(x >> 32)), "v"(acc));
#endif
  }
  return (int)acc;
}
// a 32-byte descriptor in registers: row i of an array of them, and its distance to row c of another
struct Desc256 { unsigned long long w[4]; };
__device__ __forceinline__ Desc256 load_desc(const uint8_t* base, int i) {
  const unsigned long long* D = reinterpret_cast<const unsigned long long*>(base + (size_t)i * 32);
  return Desc256{{D[0], D[1], D[2], D[3]}};
}
__device__ __forceinline__ int desc_dist(const Desc256& d, const uint8_t* base, int c) {
  return hamming256(d.w, reinterpret_cast<const unsigned long long*>(base + (size_t)c * 32));
}
__device__ __forceinline__ int desc_dist(const Desc256& a, const Desc256& b) { return hamming256(a.w, b.w); }

// A workgroup owns 64 query descriptors (one per lane, 4 x u64 in VGPRs).  Its four waves split the train set
// into four contiguous index ranges; inside a wave the train descriptor address is wave-uniform, so it is
// fetched with scalar loads and broadcast to the 64 lanes.  Best and second-best are tracked on packed words
// (distance << 16 | train index): min() then implements the reference's "strict '<', first minimum wins" and the
// second-best is the second smallest word, whose distance part is the second smallest distance counted with
// multiplicity.  The four partial results are merged through LDS with the same two operations.
// grid = (ceil(cap/64), n_pairs), block = 256.  Requires train counts < 65536.
// (All three scans: a key of distance 256 - a complement - orders below kNone but is no match: the selection starts at 256 with
// strict '<', so the index written for it is -1.)
__device__ __forceinline__ void bf_track(uint32_t& best, uint32_t& second, uint32_t cur) {
  // best <= second always: the new second is the median of (best, cur, second) - one v_med3_u32 instead of max + min
#ifdef RGBL_EMU
  const uint32_t hi = best > cur ? best : cur;
  second = second < hi ? second : hi;
#else
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(second) : "v"(best), "v"(cur), "v"(second));
#endif
  best = best < cur ? best : cur;
}

__global__ __launch_bounds__(256) void k_hamming_bf(const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_rows,
                                                    int cap, const int32_t* __restrict__ pair_a,
                                                    const int32_t* __restrict__ pair_b, int32_t* __restrict__ best_idx,
                                                    int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist) {
  __shared__ uint32_t s_best[4][64], s_second[4][64];
  const int p = blockIdx.y;
  const int fa = pair_a ? pair_a[p] : 0, fb = pair_b ? pair_b[p] : 1;
  const int na = n_rows[fa], nb = n_rows[fb];
  if ((int)blockIdx.x * 64 >= na) return;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());  // make the train range provably wave-uniform
  const int i = blockIdx.x * 64 + lane;
  const bool valid = i < na;
  const unsigned long long* A = reinterpret_cast<const unsigned long long*>(desc + ((size_t)fa * cap + (valid ? i : 0)) * 32);
  const unsigned long long* B = reinterpret_cast<const unsigned long long*>(desc + (size_t)fb * cap * 32);
  const unsigned long long q[4] = {A[0], A[1], A[2], A[3]};
  const int chunk = (nb + 3) >> 2;
  const int j0 = wave * chunk, j1 = imin(j0 + chunk, nb);
  const uint32_t kNone = (256u << 16) | 0xffffu;
  uint32_t best = kNone, second = kNone;
  int j = j0;
  for (; j + 8 <= j1; j += 8) {
    const unsigned long long* t = B + 4 * (size_t)j;
    unsigned long long tt[32];  // the eight train descriptors first (wave-uniform: four s_load_dwordx16), then the arithmetic
#pragma unroll
    for (int u = 0; u < 32; ++u) tt[u] = t[u];
    uint32_t e[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) e[u] = ((uint32_t)hamming256(q, tt + 4 * u) << 16) | (uint32_t)(j + u);
#pragma unroll
    for (int u = 0; u < 8; ++u) bf_track(best, second, e[u]);
  }
  for (; j < j1; ++j) bf_track(best, second, ((uint32_t)hamming256(q, B + 4 * (size_t)j) << 16) | (uint32_t)j);
  s_best[wave][lane] = best;
  s_second[wave][lane] = second;
  __syncthreads();
  if (wave == 0 && valid) {
    for (int w = 1; w < 4; ++w) {
      const uint32_t ob = s_best[w][lane], os = s_second[w][lane];
      const uint32_t hi = best > ob ? best : ob;
      best = best < ob ? best : ob;
      second = second < os ? second : os;
      second = second < hi ? second : hi;
    }
    const size_t o = (size_t)p * cap + i;
    best_idx[o] = best >= (256u << 16) ? -1 : (int32_t)(best & 0xffffu);
    best_dist[o] = (int32_t)(best >> 16);
    if (second_dist) second_dist[o] = (int32_t)(second >> 16);
  }
}

// ------------------------------------------------------------------------------------------------
// The same all-pairs scan on the matrix cores.  With the bits of a descriptor expanded to signed bytes,
//   train bit a -> 64 (1 - 2a),   query bit b -> -64 (1 - 2b),
// a 256-long i8 dot product is 4096 (#different - #equal) = 8192 * hamming - 2^20: v_mfma_i32_32x32x32_i8 delivers, per
// instruction, 32 of the 256 bit positions of 32 train x 32 query pairs, eight chained instructions the whole distance.
// The accumulator starts at 2^20 + (row of the tile), so what comes out IS the tracking key of k_hamming_bf - distance
// above the index, here (distance << 13 | row) - and the epilogue is v_med3 + v_min per pair, nothing else.
//   * Tile t's rows are 32 t + row; instead of adding 32 t to 16 accumulators the two running keys of a lane are lowered by
//     32 per tile (signed compares), which orders (distance, index) pairs exactly as the absolute keys would; 13 index bits
//     = sweeps of 8192 train descriptors, decoded and merged into (distance << 16 | index) words after each sweep.
//   * The position of a bit inside the K = 256 sum is free as long as both operands agree, so the expansion is chosen for
//     the VALU: dword w of a descriptor feeds MFMA step w, and byte c of its q-th expanded dword is bit 8c + q of it:
//     ((x << (7 - q)) & 0x80808080) | 0x40404040 (0xC0 = -64, 0x40 = +64), two operations per four operand bytes.
//   * Query tiles (the B operand, the D columns) live in VGPRs for the whole scan: 64 queries per wave, 256 per workgroup.
//     Train rows are expanded once per workgroup into LDS, 64 rows per stage, double buffered (one barrier per stage), rows
//     272 B apart so that the 16-byte fragment reads of a wave spread over all banks; every fragment feeds two MFMAs.
// D layout (gfx950, all 32 x 32 shapes): lane l holds column l & 31, register r row (r & 3) + 8 (r >> 2) + 4 (l >> 5).
// grid = (ceil(cap / 256), n_pairs), block = 256.  Same arguments and results as k_hamming_bf.
constexpr int kBfQueriesPerBlock = 256;
constexpr int kBfStageRows = 64;
constexpr int kBfRowBytes = 272;
constexpr int kBfSweep = 8192;
constexpr int kBfIdle = 0x3fffffff;

__device__ __forceinline__ v4i bf_expand4(uint32_t x, int q0) {
  v4i r;
  r[0] = (int)(((x << (7 - q0)) & 0x80808080u) | 0x40404040u);
  r[1] = (int)(((x << (6 - q0)) & 0x80808080u) | 0x40404040u);
  r[2] = (int)(((x << (5 - q0)) & 0x80808080u) | 0x40404040u);
  r[3] = (int)(((x << (4 - q0)) & 0x80808080u) | 0x40404040u);
  return r;
}
__device__ __forceinline__ void bf_track_rel(int& best, int& second, int cur) {
#ifdef RGBL_EMU
  const int hi = best > cur ? best : cur;
  second = second < hi ? second : hi;
#else
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(second) : "v"(best), "v"(cur), "v"(second));
#endif
  best = best < cur ? best : cur;
}
__device__ __forceinline__ void bf_merge(uint32_t& best, uint32_t& second, uint32_t ob, uint32_t os) {
  const uint32_t hi = best > ob ? best : ob;
  best = best < ob ? best : ob;
  second = second < os ? second : os;
  second = second < hi ? second : hi;
}

__global__ __launch_bounds__(256) void k_hamming_mfma(const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_rows,
                                                      int cap, const int32_t* __restrict__ pair_a,
                                                      const int32_t* __restrict__ pair_b, int32_t* __restrict__ best_idx,
                                                      int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[2][kBfStageRows * kBfRowBytes];
  // grid = xcd_grid(query blocks, pairs) (common.h): the query blocks of a pair share an XCD's L2 and with it the train set
  const int p = xcd_frame();
  const int fa = pair_a ? pair_a[p] : 0, fb = pair_b ? pair_b[p] : 1;
  const int na = n_rows[fa], nb = n_rows[fb];
  const int q_base = xcd_item() * kBfQueriesPerBlock;
  if (q_base >= na) return;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int col = lane & 31, half = lane >> 5;
  const bool wave_has_queries = q_base + wave * 64 < na;

  // query fragments: two 32-column tiles, eight K steps each
  v4i bq[2][8];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int qi = q_base + wave * 64 + ct * 32 + col;
    const uint4* src = reinterpret_cast<const uint4*>(desc + ((size_t)fa * cap + (qi < na ? qi : 0)) * 32);
    const uint4 lo = src[0], hi = src[1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int s = 0; s < 8; ++s) bq[ct][s] = bf_expand4(~x[s], 4 * half);
  }
  v16i c_init;
#pragma unroll
  for (int r = 0; r < 16; ++r) c_init[r] = (1 << 20) + (r & 3) + 8 * (r >> 2) + 4 * half;

  const uint32_t* __restrict__ train = reinterpret_cast<const uint32_t*>(desc + (size_t)fb * cap * 32);
  const uint32_t kNone = (256u << 16) | 0xffffu;
  uint32_t out_best[2] = {kNone, kNone}, out_second[2] = {kNone, kNone};

  // stage s of the whole scan = train rows [64 s, 64 s + 64); work-item tid expands dwords tid and tid + 256 of it
  const int n_stages = (nb + kBfStageRows - 1) / kBfStageRows;
  auto load_stage = [&](int stage, uint32_t& x0, uint32_t& x1) {
    const int d0 = stage * (kBfStageRows * 8) + tid, d1 = d0 + 256;
    x0 = (d0 >> 3) < nb ? train[d0] : 0u;
    x1 = (d1 >> 3) < nb ? train[d1] : 0u;
  };
  uint32_t nx0 = 0, nx1 = 0;
  if (n_stages > 0) load_stage(0, nx0, nx1);
  int best[2] = {kBfIdle, kBfIdle}, second[2] = {kBfIdle, kBfIdle};
  int tiles_in_sweep = 0;
  auto close_sweep = [&](int sweep_base) {
    // relative keys -> (distance << 16 | absolute index), folded into the results of the earlier sweeps
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int off = 32 * (tiles_in_sweep - 1);
      const int kb = best[ct] + off, ks = second[ct] + off;
      const uint32_t wb = kb >= (257 << 13) ? kNone : ((uint32_t)(kb >> 13) << 16) | (uint32_t)(sweep_base + (kb & 8191));
      const uint32_t ws = ks >= (257 << 13) ? kNone : ((uint32_t)(ks >> 13) << 16) | (uint32_t)(sweep_base + (ks & 8191));
      bf_merge(out_best[ct], out_second[ct], wb, ws);
      best[ct] = second[ct] = kBfIdle;
    }
    tiles_in_sweep = 0;
  };
  for (int stage = 0; stage < n_stages; ++stage) {
    uint8_t* buf = s_rows[stage & 1];
    const uint32_t x0 = nx0, x1 = nx1;
    if (stage + 1 < n_stages) load_stage(stage + 1, nx0, nx1);
    {
      uint8_t* r0 = buf + (tid >> 3) * kBfRowBytes + (tid & 7) * 32;
      uint8_t* r1 = r0 + 32 * kBfRowBytes;
      *reinterpret_cast<v4i*>(r0) = bf_expand4(x0, 0);
      *reinterpret_cast<v4i*>(r0 + 16) = bf_expand4(x0, 4);
      *reinterpret_cast<v4i*>(r1) = bf_expand4(x1, 0);
      *reinterpret_cast<v4i*>(r1 + 16) = bf_expand4(x1, 4);
    }
    __syncthreads();
    if (!wave_has_queries) continue;
#pragma unroll 1
    for (int rt = 0; rt < 2; ++rt) {
      const int row0 = stage * kBfStageRows + rt * 32;  // first train row of the tile
      if (row0 >= nb) break;
      const uint8_t* frag = buf + (rt * 32 + col) * kBfRowBytes + half * 16;
      v16i acc0 = c_init, acc1 = c_init;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const v4i a = *reinterpret_cast<const v4i*>(frag + s * 32);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[0][s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[1][s], acc1, 0, 0, 0);
      }
      best[0] -= 32; second[0] -= 32; best[1] -= 32; second[1] -= 32;
      ++tiles_in_sweep;
      if (row0 + 32 <= nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { bf_track_rel(best[0], second[0], acc0[r]); bf_track_rel(best[1], second[1], acc1[r]); }
      } else {  // the last tile of the train set: rows beyond it never win
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool live = row0 + (r & 3) + 8 * (r >> 2) + 4 * half < nb;
          bf_track_rel(best[0], second[0], live ? acc0[r] : kBfIdle);
          bf_track_rel(best[1], second[1], live ? acc1[r] : kBfIdle);
        }
      }
      if (((row0 + 32) & (kBfSweep - 1)) == 0) close_sweep(row0 + 32 - kBfSweep);
    }
  }
  if (!wave_has_queries) return;
  if (tiles_in_sweep > 0) close_sweep(((nb - 1) / kBfSweep) * kBfSweep);
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    // the two halves of the wave hold the same columns, interleaved groups of four rows
    const uint32_t ob = __shfl_xor(out_best[ct], 32), os = __shfl_xor(out_second[ct], 32);
    bf_merge(out_best[ct], out_second[ct], ob, os);
    const int qi = q_base + wave * 64 + ct * 32 + col;
    if (half == 0 && qi < na) {
      const size_t o = (size_t)p * cap + qi;
      best_idx[o] = out_best[ct] >= (256u << 16) ? -1 : (int32_t)(out_best[ct] & 0xffffu);
      best_dist[o] = (int32_t)(out_best[ct] >> 16);
      if (second_dist) second_dist[o] = (int32_t)(out_second[ct] >> 16);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The same scan once more, on gfx950's block-scaled FP4 matrix-core instruction (v_mfma_scale_f32_32x32x64_f8f6f4 with
// E2M1 operands: 64 bit positions per instruction, twice the i8 rate, half the operand bytes).  A descriptor bit becomes the
// four-bit float +-4 (0x6 / 0xE): train bit a -> 4 (1 - 2a), query bit b -> -4 (1 - 2b); both operands carry the block scale
// 2^4 (E8M0 byte 131), so a product is +-4096 and the 256-long sum is 8192 * hamming - 2^20 - the numbers of the i8 form,
// exact in the f32 accumulator (all values are integers below 2^22).  The accumulator starts at 2^20 + row, the tracking
// key comes out as a float and is tracked with two v_med3_f32 per value (bf_track_rel_f).  Dword w of a descriptor is the 32 values one lane
// group feeds to step w / 2 (group w & 1); which bit lands in which nibble of the group does not matter as long as train
// and query agree.  Everything else - query tiles in VGPRs, kBfStageRowsF4 train rows per double-buffered LDS stage, relative keys,
// sweeps - as in k_hamming_mfma.  grid = (ceil(cap / 256), n_pairs), block = 256.
constexpr int kBfStageRowsF4 = 64;  // train rows per LDS stage of k_hamming_fp4: a multiple of 32, the kernel follows it
constexpr int kBfStageLoadsF4 = kBfStageRowsF4 * 8 / 256;  // dwords of a stage per work-item (32 rows apart)
constexpr int kBfRowBytesF4 = 144;  // 128 bytes of nibbles + 16: the 16-byte fragment reads of a wave spread over the banks
constexpr float kBfIdleF = 1073741824.f;

__device__ __forceinline__ v4i bf_expand_fp4(uint32_t x) {  // bit j of x -> nibble j: 0x6 (+4) or 0xE (-4)
  v4i r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t t = (x >> (8 * i)) & 0xffu;
    t = (t | (t << 12)) & 0x000f000fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    r[i] = (int)(0x66666666u | (t << 3));
  }
  return r;
}
// Two vector instructions per accumulator value, both visible to the compiler: it is the compiler's hazard recogniser that
// puts the wait states between the last MFMA of a tile and the first read of its accumulator, and it does not look into
// inline assembly.  min(a, b) is written as med3(a, b, -inf): fminf() under strict floating-point rules costs a
// canonicalising v_max_f32 x, x in front of every v_min_f32, the median intrinsic takes its operands as they are (no NaNs
// here, all values are integers).  `neg_inf` is -infinity in a register the compiler cannot see through (bf_neg_inf).
__device__ __forceinline__ float bf_neg_inf() {
  float v = -INFINITY;
#ifndef RGBL_EMU
  asm("" : "+s"(v));  // opaque: keeps med3(a, b, -inf) from being folded back into a canonicalising minimum
#endif
  return v;
}
__device__ __forceinline__ void bf_track_rel_f(float& best, float& second, float cur, float neg_inf) {
#ifdef RGBL_EMU
  const float hi = best > cur ? best : cur;
  second = second < hi ? second : hi;
  best = best < cur ? best : cur;
#else
  second = __builtin_amdgcn_fmed3f(best, cur, second);  // best <= second always: the median is the new second
  best = __builtin_amdgcn_fmed3f(best, cur, neg_inf);
#endif
}

// The scheduling directives of bf_tile_f4 (LLVM SchedGroupMask: VALU 0x2, MFMA 0x8, DS read 0x100); the emulator has no scheduler.
#ifdef RGBL_EMU
#define BF_SCHED_FENCE() ((void)0)
#define BF_SCHED_GROUP(mask, n, id) ((void)0)
#define BF_PIN(best, second) ((void)0)
#else
#define BF_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define BF_SCHED_GROUP(mask, n, id) __builtin_amdgcn_sched_group_barrier(mask, n, id)
// the tracking instructions have no side effects, so nothing orders them against a fence until their values pass through a
// statement that has some: an empty one on the running pair (never on an accumulator: see bf_track_rel_f)
#define BF_PIN(best, second) asm volatile("" : "+v"(best), "+v"(second))
#endif
constexpr int kBfScaleF4 = 131;  // E8M0: 2^(131 - 127) = 16 per operand
__device__ __forceinline__ v16f bf_mfma_f4(const v4i& a, const v8i& b, const v16f& c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b, c, 4, 4, 0, kBfScaleF4, 0, kBfScaleF4);
}
// One tile of 32 train rows (fragments a[0..3]) against the wave's two query tiles, as a two-phase software pipeline: a wave is
// in-order, so its tracking only runs beside its matrix instructions if it stands between them in the instruction stream.
//   phase A: the four MFMAs of acc0 (queries 0 - 31) for this tile, between them the tracking of acc1 of the PREVIOUS tile;
//   phase B: the four MFMAs of acc1 (queries 32 - 63) for this tile, between them the tracking of acc0 of this tile.
// acc1 therefore leaves a tile untracked (the caller keeps it, across stage barriers too, and drains it at the end of a sweep and
// of the scan).  Each running pair is lowered by 32 once per tile, right before that tile's values meet it.  Only full tiles
// come here: the partial last stage of a train set is scanned behind the stage loop, where its mask is.
// kPrefetch: every fragment register is reloaded from frag_next (the next tile of the stage) behind its last MFMA.
// Fences keep the phases apart, the groups pin MFMA / 8 tracking instructions / MFMA ... inside a phase.  Neither accumulator
// set is ever copied: acc1 is dead when phase B's first MFMA writes it, acc0 when the next tile's phase A does.
template <bool kPrefetch>
__device__ __forceinline__ void bf_tile_f4(const uint8_t* frag_next, v4i (&a)[4], const v8i (&bq)[2][4], const v16f& c_init, v16f& acc0, v16f& acc1,
                                           float (&best)[2], float (&second)[2], float neg_inf) {
  best[1] -= 32.f; second[1] -= 32.f;
  BF_PIN(best[1], second[1]);
  BF_SCHED_FENCE();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc0 = bf_mfma_f4(a[s], bq[0][s], s == 0 ? c_init : acc0);
#pragma unroll
    for (int r = 4 * s; r < 4 * s + 4; ++r) bf_track_rel_f(best[1], second[1], acc1[r], neg_inf);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) { BF_SCHED_GROUP(0x008, 1, 1); BF_SCHED_GROUP(0x002, 8, 1); }
  BF_PIN(best[1], second[1]);
  BF_SCHED_FENCE();
  best[0] -= 32.f; second[0] -= 32.f;
  BF_PIN(best[0], second[0]);
  BF_SCHED_FENCE();
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc1 = bf_mfma_f4(a[s], bq[1][s], s == 0 ? c_init : acc1);
    if (kPrefetch) a[s] = *reinterpret_cast<const v4i*>(frag_next + s * 32);
#pragma unroll
    for (int r = 4 * s; r < 4 * s + 4; ++r) bf_track_rel_f(best[0], second[0], acc0[r], neg_inf);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    BF_SCHED_GROUP(0x008, 1, 2);
    if (kPrefetch) BF_SCHED_GROUP(0x100, 1, 2);
    BF_SCHED_GROUP(0x002, 8, 2);
  }
  BF_PIN(best[0], second[0]);
  BF_SCHED_FENCE();
}

__global__ __launch_bounds__(256, 4) void k_hamming_fp4(const uint8_t* __restrict__ desc, const int32_t* __restrict__ n_rows,
                                                     int cap, const int32_t* __restrict__ pair_a,
                                                     const int32_t* __restrict__ pair_b, int32_t* __restrict__ best_idx,
                                                     int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist,
                                                     int splits, uint32_t* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[2][kBfStageRowsF4 * kBfRowBytesF4];
  __shared__ uint32_t s_lut[256];  // byte -> its eight nibbles: the train rows are expanded with four table reads per dword
  // splits > 1 (one pair per call, rgbl_hamming_bf): the launch's frame index is a slice of the train set instead of a pair;
  // every slice leaves its packed best / second per query in `partial`, k_hamming_merge folds them (a frame against a frame is
  // 8 query blocks: alone they occupy 8 of 256 CUs for 43 us)
  const int split = splits > 1 ? xcd_frame() : 0;
  const int p = splits > 1 ? 0 : xcd_frame();
  const int fa = pair_a ? pair_a[p] : 0, fb = pair_b ? pair_b[p] : 1;
  const int na = n_rows[fa], nb = n_rows[fb];
  const int q_base = xcd_item() * kBfQueriesPerBlock;
  if (q_base >= na) return;
  const int tid = threadIdx.x, lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(wave_id());
  const int col = lane & 31, half = lane >> 5;
  const bool wave_has_queries = q_base + wave * 64 < na;
  s_lut[tid] = (uint32_t)bf_expand_fp4((uint32_t)tid)[0];  // the first barrier of the stage loop publishes it

  // query fragments: two 32-column tiles, four K steps each
  v8i bq[2][4];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int qi = q_base + wave * 64 + ct * 32 + col;
    const uint4* src = reinterpret_cast<const uint4*>(desc + ((size_t)fa * cap + (qi < na ? qi : 0)) * 32);
    const uint4 lo = src[0], hi = src[1];
    // the lane's dword of every step picked value by value: an array indexed by `half` ends up in scratch memory
    const uint32_t x[4] = {half ? lo.y : lo.x, half ? lo.w : lo.z, half ? hi.y : hi.x, half ? hi.w : hi.z};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const v4i e = bf_expand_fp4(~x[s]);
      bq[ct][s] = v8i{e[0], e[1], e[2], e[3], 0, 0, 0, 0};
    }
  }
  v16f c_init;
#pragma unroll
  for (int r = 0; r < 16; ++r) c_init[r] = (float)((1 << 20) + (r & 3) + 8 * (r >> 2) + 4 * half);

  const uint32_t* __restrict__ train = reinterpret_cast<const uint32_t*>(desc + (size_t)fb * cap * 32);
  const uint32_t kNone = (256u << 16) | 0xffffu;
  uint32_t out_best[2] = {kNone, kNone}, out_second[2] = {kNone, kNone};

  // stage s of the whole scan = kBfStageRowsF4 train rows; work-item tid expands dwords tid, tid + 256, ... of it
  const int all_stages = (nb + kBfStageRowsF4 - 1) / kBfStageRowsF4;
  const int stages_per = (all_stages + splits - 1) / (splits > 1 ? splits : 1);
  const int s_begin = split * stages_per, n_stages = imin(all_stages, s_begin + stages_per);  // this launch slice: stages [s_begin, n_stages)
  auto load_stage = [&](int stage, uint32_t (&x)[kBfStageLoadsF4]) {
#pragma unroll
    for (int k = 0; k < kBfStageLoadsF4; ++k) {
      const int d = stage * (kBfStageRowsF4 * 8) + k * 256 + tid;
      x[k] = (d >> 3) < nb ? train[d] : 0u;
    }
  };
  uint32_t nx[kBfStageLoadsF4] = {};
  if (n_stages > s_begin) load_stage(s_begin, nx);
  float best[2] = {kBfIdleF, kBfIdleF}, second[2] = {kBfIdleF, kBfIdleF};
  const float neg_inf = bf_neg_inf();
  int tiles_in_sweep = 0;
  int sweep_start = s_begin * kBfStageRowsF4;  // first train row of the sweep in progress
  auto close_sweep = [&](int sweep_base) {
    // relative keys -> (distance << 16 | absolute index), folded into the results of the earlier sweeps
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const float off = (float)(32 * (tiles_in_sweep - 1));
      const int kb = (int)(best[ct] + off), ks = (int)(second[ct] + off);  // exact: integers below 2^31 / idle 2^30 + small
      const uint32_t wb = kb >= (257 << 13) ? kNone : ((uint32_t)(kb >> 13) << 16) | (uint32_t)(sweep_base + (kb & 8191));
      const uint32_t ws = ks >= (257 << 13) ? kNone : ((uint32_t)(ks >> 13) << 16) | (uint32_t)(sweep_base + (ks & 8191));
      bf_merge(out_best[ct], out_second[ct], wb, ws);
      best[ct] = second[ct] = kBfIdleF;
    }
    tiles_in_sweep = 0;
  };
  // acc1 is the pending tile of bf_tile_f4: it lives across tiles and stage barriers; before the first tile of a sweep it holds
  // idle keys, which the tracker ignores (the pair is lowered once more than it has tiles then, while it holds nothing but idle).
  v16f acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc1[r] = kBfIdleF;
  auto drain = [&]() {  // track the pending tile on its own (end of a sweep, end of the full stages): phase A without MFMAs
    best[1] -= 32.f; second[1] -= 32.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) bf_track_rel_f(best[1], second[1], acc1[r], neg_inf);
  };
  constexpr int kTiles = kBfStageRowsF4 / 32;
  const uint8_t* tail = nullptr;
  static_assert(kBfSweep % kBfStageRowsF4 == 0, "a sweep closes at the end of a stage");
  for (int stage = s_begin; stage < n_stages; ++stage) {
    uint8_t* buf = s_rows[stage & 1];
    uint32_t x[kBfStageLoadsF4];
#pragma unroll
    for (int k = 0; k < kBfStageLoadsF4; ++k) x[k] = nx[k];
    if (stage + 1 < n_stages) load_stage(stage + 1, nx);
    {
      uint8_t* r0 = buf + (tid >> 3) * kBfRowBytesF4 + (tid & 7) * 16;
#pragma unroll
      for (int k = 0; k < kBfStageLoadsF4; ++k) {
        v4i* dst = reinterpret_cast<v4i*>(r0 + k * 32 * kBfRowBytesF4);
        if (stage == s_begin) *dst = bf_expand_fp4(x[k]);  // the table is not published yet
        else *dst = v4i{(int)s_lut[x[k] & 0xff], (int)s_lut[(x[k] >> 8) & 0xff], (int)s_lut[(x[k] >> 16) & 0xff], (int)s_lut[x[k] >> 24]};
      }
    }
    __syncthreads();
    if (!wave_has_queries) continue;
    const int row_s = stage * kBfStageRowsF4;  // first train row of the stage
    const uint8_t* frag = buf + col * kBfRowBytesF4 + half * 16;
    v4i a[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {  // in the order the MFMAs take them (the fences keep it), so that the first waits for one read only
      a[s] = *reinterpret_cast<const v4i*>(frag + s * 32);
      BF_SCHED_FENCE();
    }
    // The partial stage of a train set goes behind the loop.  Leaving a loop that holds a barrier is safe here because a partial
    // stage is always the last one this launch scans: row_s + kBfStageRowsF4 > nb means stage == all_stages - 1, and n_stages <=
    // all_stages, so stage == n_stages - 1 and the waves without queries (which `continue` above) meet no further barrier either.
    if (row_s + kBfStageRowsF4 > nb) { tail = buf; break; }
    // straight-line tiles, each requests the fragments of the next
#pragma unroll
    for (int rt = 0; rt < kTiles; ++rt) {
      if (rt + 1 < kTiles) bf_tile_f4<true>(frag + (rt + 1) * 32 * kBfRowBytesF4, a, bq, c_init, acc0, acc1, best, second, neg_inf);
      else bf_tile_f4<false>(frag, a, bq, c_init, acc0, acc1, best, second, neg_inf);
    }
    tiles_in_sweep += kTiles;
    if (tiles_in_sweep == kBfSweep / 32) {
      drain();
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[r] = kBfIdleF;
      close_sweep(sweep_start);
      sweep_start = row_s + kBfStageRowsF4;
    }
  }
  if (!wave_has_queries) return;
  if (tiles_in_sweep > 0) drain();
  if (tail) {
    // at most kTiles tiles, the last one masked (rows beyond the train set never win): no barrier follows, nothing is left pending,
    // so they are tracked where they are computed, with accumulators of their own.  `tail` was set in stage n_stages - 1 (see the
    // break above), hence the first row below.
#pragma unroll 1
    for (int row0 = (n_stages - 1) * kBfStageRowsF4; row0 < nb; row0 += 32, tail += 32 * kBfRowBytesF4) {
      const uint8_t* frag = tail + col * kBfRowBytesF4 + half * 16;
      v16f t0 = c_init, t1 = c_init;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const v4i a = *reinterpret_cast<const v4i*>(frag + s * 32);
        t0 = bf_mfma_f4(a, bq[0][s], t0);
        t1 = bf_mfma_f4(a, bq[1][s], t1);
      }
      best[0] -= 32.f; second[0] -= 32.f; best[1] -= 32.f; second[1] -= 32.f;
      ++tiles_in_sweep;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool live = row0 + (r & 3) + 8 * (r >> 2) + 4 * half < nb;
        bf_track_rel_f(best[0], second[0], live ? t0[r] : kBfIdleF, neg_inf);
        bf_track_rel_f(best[1], second[1], live ? t1[r] : kBfIdleF, neg_inf);
      }
    }
  }
  if (tiles_in_sweep > 0) close_sweep(sweep_start);
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    // the two halves of the wave hold the same columns, interleaved groups of four rows
    const uint32_t ob = __shfl_xor(out_best[ct], 32), os = __shfl_xor(out_second[ct], 32);
    bf_merge(out_best[ct], out_second[ct], ob, os);
    const int qi = q_base + wave * 64 + ct * 32 + col;
    if (half == 0 && qi < na) {
      if (splits > 1) {
        uint32_t* o = partial + ((size_t)split * na + qi) * 2;
        o[0] = out_best[ct]; o[1] = out_second[ct];
      } else {
        const size_t o = (size_t)p * cap + qi;
        best_idx[o] = out_best[ct] >= (256u << 16) ? -1 : (int32_t)(out_best[ct] & 0xffffu);
        best_dist[o] = (int32_t)(out_best[ct] >> 16);
        if (second_dist) second_dist[o] = (int32_t)(out_second[ct] >> 16);
      }
    }
  }
}

// folds the slices' packed (distance << 16 | index) best / second of every query (k_hamming_fp4 with splits > 1)
__global__ __launch_bounds__(256) void k_hamming_merge(const uint32_t* __restrict__ partial, int na, int splits, int32_t* __restrict__ best_idx,
                                                       int32_t* __restrict__ best_dist, int32_t* __restrict__ second_dist) {
  const int qi = blockIdx.x * 256 + threadIdx.x;
  if (qi >= na) return;
  const uint32_t kNone = (256u << 16) | 0xffffu;
  uint32_t b = kNone, s2 = kNone;
  for (int sp = 0; sp < splits; ++sp) {
    const uint32_t* o = partial + ((size_t)sp * na + qi) * 2;
    bf_merge(b, s2, o[0], o[1]);
  }
  best_idx[qi] = b >= (256u << 16) ? -1 : (int32_t)(b & 0xffffu);
  best_dist[qi] = (int32_t)(b >> 16);
  if (second_dist) second_dist[qi] = (int32_t)(s2 >> 16);
}


// ------------------------------------------------------------------------------------------------
// MapPoint::ComputeDistinctiveDescriptors (/root/reference/src/MapPoint.cc:329-403) for a batch of map points: among the
// N descriptors that observe a point, the one with the least median Hamming distance to all N (its own 0 included; median =
// sorted row[(size_t)(0.5 * (N - 1))]; strict '<' over the rows, so the first minimum wins).
// One wave per point, one row per lane (rows in chunks of 64); the other descriptor of a pair is wave-uniform and comes
// through scalar loads.  The k-th smallest of a row is found by bisection on the value range 0..256 (9 counting passes that
// recompute the distances: N is a few dozen, nothing is stored).
// grid = points, block = 64
__global__ __launch_bounds__(64) void k_distinctive(const uint8_t* __restrict__ desc, const int32_t* __restrict__ off, int32_t* __restrict__ best) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int b = off[p], n = off[p + 1] - b;
  if (n <= 0) { if (lane == 0) best[p] = -1; return; }
  const unsigned long long* D = reinterpret_cast<const unsigned long long*>(desc) + 4 * (size_t)b;
  const int k = (n - 1) >> 1;  // (size_t)(0.5 * (N - 1))
  uint32_t wbest = 0xffffffffu;  // median << 16 | row
  for (int r0 = 0; r0 < n; r0 += 64) {
    const int i = r0 + lane;
    const bool live = i < n;
    const unsigned long long* Q = D + 4 * (size_t)(live ? i : 0);
    const unsigned long long q[4] = {Q[0], Q[1], Q[2], Q[3]};
    int lo = 0, hi = 256;
    for (int it = 0; it < 9; ++it) {  // 257 possible values
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int j = 0; j < n; ++j) c += hamming256(q, D + 4 * (size_t)j) <= mid ? 1 : 0;
      if (c >= k + 1) hi = mid; else lo = mid + 1;
    }
    uint32_t key = live ? ((uint32_t)lo << 16) | (uint32_t)i : 0xffffffffu;
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)key, m); key = o < key ? o : key; }
    wbest = key < wbest ? key : wbest;
  }
  if (lane == 0) best[p] = (int32_t)(wbest & 0xffffu);
}

// The searches over the vocabulary nodes two FeatureVectors share (SearchForTriangulation here, SearchByBoW further down) launch
// one workgroup per shared node: node_span() is where workgroup blockIdx.x finds its two buckets.
struct NodePairsDev {
  const int32_t *off1, *feat1, *off2, *feat2;  // CSR buckets
  const int32_t *pair_n1, *pair_n2;            // matched node pairs (indices into off1 / off2)
};
struct NodeSpan { int b1, n1, b2, n2; };       // the buckets are feat1[b1 .. b1 + n1) and feat2[b2 .. b2 + n2)
__device__ __forceinline__ NodeSpan node_span(const NodePairsDev& N) {
  const int a = N.pair_n1[blockIdx.x], b = N.pair_n2[blockIdx.x];
  const int b1 = N.off1[a], b2 = N.off2[b];
  return NodeSpan{b1, N.off1[a + 1] - b1, b2, N.off2[b + 1] - b2};
}

struct TriDev {
  const uint8_t *desc1, *desc2;
  const float *xy1, *xy2;
  const int32_t* oct2;
  const float *ur1, *ur2;
  const uint8_t *mp1, *mp2;
  NodePairsDev fv;
  float F[9], ep[2];
  const float *scale2, *sigma2;
  int only_stereo, coarse;
  int32_t* matches12;
};

// grid = number of node ids present in both feature vectors, block = 256.
// A first-image feature keeps the LAST second-image feature of the node's bucket with the smallest distance <= TH_LOW among those that
// pass the tests (":1075 if(dist>TH_LOW || dist>bestDist) continue" lets an equal distance replace the best) - the tests do not
// depend on what was found before, and nothing is handed from one first-image feature to the next (vbMatched2 is never set in this
// version, :1135): every pair is independent.  Round 6: a work-item per first-image feature walked the bucket through ~4 dependent
// global loads per candidate (38 us for 2000 x 2000 features in ~100 nodes, 20 work-items of a workgroup busy).  Now both buckets
// are staged in LDS by all 256 work-items at once (kTriCap entries each; longer buckets read the rest from global memory), a WAVE
// takes a first-image feature, its lanes the candidates, and one DPP minimum over (distance << 26 | 2^26 - 1 - position) names the match.
constexpr int kTriCap = 256;
struct TriEntry {
  Desc256 d;
  float x, y;
  int32_t idx;
  int32_t oct_flags;  // octave | stereo << 8 | skip << 9 (holds a map point, or not stereo under only_stereo)
};
static_assert(sizeof(TriEntry) == 48, "k_search_triangulation's 24 576 bytes of LDS are 2 * kTriCap entries of 48 bytes");
__device__ __forceinline__ TriEntry tri_load(const TriDev& T, bool second, int idx) {
  TriEntry e;
  e.d = load_desc(second ? T.desc2 : T.desc1, idx);
  const float* xy = second ? T.xy2 : T.xy1;
  e.x = xy[2 * idx]; e.y = xy[2 * idx + 1];
  e.idx = idx;
  const bool stereo = (second ? T.ur2 : T.ur1)[idx] >= 0;
  const bool skip = (second ? T.mp2 : T.mp1)[idx] != 0 || (T.only_stereo && !stereo);
  e.oct_flags = (second ? T.oct2[idx] : 0) | (stereo ? 0x100 : 0) | (skip ? 0x200 : 0);
  return e;
}
__global__ __launch_bounds__(256) void k_search_triangulation(TriDev T) {
  __shared__ TriEntry s_1[kTriCap], s_2[kTriCap];
  const int tid = threadIdx.x, lane = lane_id();
  const NodeSpan S = node_span(T.fv);
  const int b1 = S.b1, n1 = S.n1, b2 = S.b2, n2 = S.n2;
  if (tid < n1) s_1[tid] = tri_load(T, false, T.fv.feat1[b1 + tid]);
  if (tid < n2) s_2[tid] = tri_load(T, true, T.fv.feat2[b2 + tid]);
  __syncthreads();
  for (int p = wave_id(); p < n1; p += 4) {   // wave-uniform
    TriEntry e1;
    if (p < kTriCap) e1 = s_1[p]; else e1 = tri_load(T, false, T.fv.feat1[b1 + p]);
    if (e1.oct_flags & 0x200) continue;
    const bool stereo1 = (e1.oct_flags & 0x100) != 0;
    // epipolar line of kp1 in image 2 (Pinhole.cpp:115-117), constant over the candidates
    const float la = e1.x * T.F[0] + e1.y * T.F[3] + T.F[6];
    const float lb = e1.x * T.F[1] + e1.y * T.F[4] + T.F[7];
    const float lc = e1.x * T.F[2] + e1.y * T.F[5] + T.F[8];
    const float den = la * la + lb * lb;
    uint32_t best = 0xffffffffu;
    for (int j = lane; j < n2; j += 64) {
      TriEntry e2;
      if (j < kTriCap) e2 = s_2[j]; else e2 = tri_load(T, true, T.fv.feat2[b2 + j]);
      if (e2.oct_flags & 0x200) continue;
      const int dist = desc_dist(e1.d, e2.d);
      if (dist > 50 /* TH_LOW */) continue;
      const int oct2 = e2.oct_flags & 0xff;
      if (!stereo1 && !(e2.oct_flags & 0x100)) {
        const float ex = T.ep[0] - e2.x, ey = T.ep[1] - e2.y;
        if (ex * ex + ey * ey < 100 * T.scale2[oct2]) continue;
      }
      bool ok = T.coarse != 0;
      if (!ok && den != 0) {
        const float num = la * e2.x + lb * e2.y + lc;
        const float dsqr = __fdiv_rn(num * num, den);
        ok = (double)dsqr < 3.84 * (double)T.sigma2[oct2];  // 3.84 is a double literal in the reference
      }
      if (!ok) continue;
      const uint32_t key = ((uint32_t)dist << 26) | (uint32_t)(0x3ffffff - j);   // dist <= 50: six bits
      best = key < best ? key : best;
    }
    best = wave_min_uniform(best);
    if (lane == 0 && best != 0xffffffffu) {
      const int j = 0x3ffffff - (int)(best & 0x3ffffffu);
      T.matches12[e1.idx] = j < kTriCap ? s_2[j].idx : T.fv.feat2[b2 + j];
    }
  }
}


// ------------------------------------------------------------------------------------------------
// The per-match block of LocalMapping::CreateNewMapPoints (/root/reference/src/LocalMapping.cc:481-710) behind
// k_search_triangulation, neighbour after neighbour on one stream (rgbl_create_new_map_points): csrc/newpoint_math.h holds the
// arithmetic, this kernel the order.  ONE workgroup walks idx2[0 .. n) in tiles in ascending index - the order of
// vMatchedIndices (ORBmatcher.cc:1138-1144) - a work-item per match; the records leave compacted in that order (ballot and
// prefix inside the tile, a running base across tiles and, through D.total, across the launches of a chain).  An accepted match
// sets mask1[idx1] (mpCurrentKeyFrame->AddMapPoint, :701): the next neighbour's k_search_triangulation skips that feature.
// One workgroup, because the chain is sequential and the order is the workgroup's to keep; with the Jacobi sweeps in fp64 the
// kernel is nine tenths of a call of KITTI size (fp32 sweeps would take a tenth off) - several workgroups over the
// list are where a gain would come from.
struct NewPointsKf {
  const float *xy, *xy_raw, *ur, *depth;   // mvKeysUn[].pt, mvKeys[].pt, mvuRight, mvDepth
  const int32_t* oct;
  const float *scale, *sigma2;             // mvScaleFactors, mvLevelSigma2
  float Tcw[12], Ow[3], K[4], mb;
};
struct NewPointsDev {
  NewPointsKf k1, k2;
  NpParams P;
  int n, n_levels;
  const int32_t* idx1;   // null: entry i is feature i of key frame 1 (the chain); else explicit pairs (rgbl_triangulate_matches)
  int32_t* idx2;         // the match of entry i, -1 = none; reset to -1 once read when `reset` (the chain's matches12)
  int32_t* list;         // scratch, n entries: the matched entries in ascending order
  int reset, report_rejected, neighbour, cap;
  uint8_t* mask1;        // nullable
  rgbl_new_point* out;
  int32_t* total;        // records so far (all launches of the call)
  int32_t* per_launch;   // [0] matches, [1] records of this launch
};
__device__ __forceinline__ NpSide new_points_side(const NewPointsKf& k, int i, int n_levels) {
  NpSide S;
  for (int j = 0; j < 12; ++j) S.Tcw[j] = k.Tcw[j];
  for (int j = 0; j < 3; ++j) S.Ow[j] = k.Ow[j];
  for (int j = 0; j < 4; ++j) S.K[j] = k.K[j];
  S.mb = k.mb;
  S.u = k.xy[2 * i]; S.v = k.xy[2 * i + 1];
  S.u_raw = k.xy_raw[2 * i]; S.v_raw = k.xy_raw[2 * i + 1];
  S.uright = k.ur[i];
  S.depth = k.depth[i];
  const int o = imin(imax(k.oct[i], 0), n_levels - 1);   // a resident frame's octaves are not checked on the host
  S.sigma2 = k.sigma2[o];
  S.scale = k.scale[o];
  return S;
}
// grid = 1, block = kNewPointsBS.  Two passes: the matched entries are first listed side by side - a tile of entries holds a
// few dozen matches, and in a wave that holds one every work-item without one idles through the whole per-match block -, then
// the list is walked densely.
constexpr int kNewPointsBS = 512, kNewPointsWaves = kNewPointsBS / 64;
__global__ __launch_bounds__(kNewPointsBS) void k_new_points(NewPointsDev D) {
  __shared__ int s_cnt[kNewPointsWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int base0 = D.total[0];
  __syncthreads();   // every wave has read D.total before work-item 0 writes it
  int m = 0;         // matches listed so far
  for (int t0 = 0; t0 < D.n; t0 += kNewPointsBS) {
    const int i = t0 + tid;
    const bool has = i < D.n && D.idx2[i] >= 0;
    const unsigned long long mh = __ballot(has);
    if (lane == 0) s_cnt[w] = (int)__popcll(mh);
    __syncthreads();
    int before = 0, tile = 0;
    for (int v = 0; v < kNewPointsWaves; ++v) {
      before += v < w ? s_cnt[v] : 0;
      tile += s_cnt[v];
    }
    if (has) D.list[m + before + (int)__popcll(mh & lanemask_lt())] = i;
    m += tile;
    __syncthreads();   // s_cnt is written again in the next tile; and the list is the workgroup's to read from here on
  }
  int base = base0;
  for (int p0 = 0; p0 < m; p0 += kNewPointsBS) {
    const int p = p0 + tid;
    const bool live = p < m;
    int i1 = 0, i2 = -1;
    uint8_t st = kNpNone;
    float x3D[3] = {0.f, 0.f, 0.f};
    if (live) {
      const int i = D.list[p];
      i2 = D.idx2[i];
      if (D.reset) D.idx2[i] = -1;
      i1 = D.idx1 ? D.idx1[i] : i;
      const NpSide S1 = new_points_side(D.k1, i1, D.n_levels), S2 = new_points_side(D.k2, i2, D.n_levels);
      st = np_check(S1, S2, D.P, x3D);
    }
    const bool accepted = st >= kNpTriangulated && st <= kNpStereo2;
    const bool emit = live && (D.report_rejected || accepted);
    if (accepted && D.mask1) D.mask1[i1] = 1;
    const unsigned long long me = __ballot(emit);
    if (lane == 0) s_cnt[w] = (int)__popcll(me);
    __syncthreads();
    int before = 0, tile = 0;
    for (int v = 0; v < kNewPointsWaves; ++v) {
      before += v < w ? s_cnt[v] : 0;
      tile += s_cnt[v];
    }
    if (emit) {
      const int pos = base + before + (int)__popcll(me & lanemask_lt());
      if (pos < D.cap) {
        rgbl_new_point r;
        r.neighbour = D.neighbour; r.idx1 = i1; r.idx2 = i2;
        r.x3D[0] = x3D[0]; r.x3D[1] = x3D[1]; r.x3D[2] = x3D[2];
        r.status = st; r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
        D.out[pos] = r;
      }
    }
    base += tile;
    __syncthreads();   // s_cnt is written again in the next pass
  }
  if (tid == 0) {
    D.total[0] = base;
    D.per_launch[0] = m;
    D.per_launch[1] = base - base0;
  }
}

__global__ void k_test_np_cos_parallax(float mb, const float* __restrict__ depth, float* __restrict__ y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = np_cos_parallax_stereo(mb, depth[i]);
}

// ------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
// (/root/reference/src/ORBmatcher.cc:1676-1887, single camera) with Frame::AssignFeaturesToGrid,
// PosInGrid and GetFeaturesInArea (src/Frame.cc:475-506, 815-825, 747-813).
//
// The reference walks the LastFrame map points in index order, and a point with observations BLOCKS the feature it is
// assigned to for every later point: a sequential greedy assignment.  Three kernels:
//   k_proj_grid        one workgroup: AssignFeaturesToGrid as a counting sort
//   k_proj_candidates  work-item per map point: projection, search window, Hamming distance to every feature in the
//                      window; the VIABLE candidates (distance <= TH_HIGH - nothing else can ever be assigned) are kept
//                      as (distance, cell order, feature) keys - the minimum key is the reference's "first minimum"
//   k_proj_resolve     one workgroup resolves the greedy order in rounds: an unresolved point takes the smallest key
//                      whose feature is not held by a lower-index blocker; it is FINAL once no unresolved lower-index
//                      blocker still has that feature among its viable candidates (min_unres).  Finals commit, the
//                      rest try again.  The lowest unresolved index is final in every round, so the loop terminates,
//                      and induction over the index shows the result is the sequential one.
constexpr int kProjCand = 16;  // viable candidates kept per point; a point with more re-scans its window (kRefOverflow)
constexpr uint32_t kRefOverflow = 1u << 31;
__host__ __device__ __forceinline__ int ref_n(uint32_t r) { return (int)((r >> 26) & 31u); }
__host__ __device__ __forceinline__ uint32_t ref_start(uint32_t r) { return r & 0x3ffffffu; }
// an entry of a point's candidate list as the resolve kernels read it
__host__ __device__ __forceinline__ uint32_t cand_entry(int dist, int level, int c) { return ((uint32_t)dist << 20) | ((uint32_t)level << 16) | (uint32_t)c; }
__host__ __device__ __forceinline__ int entry_dist(uint32_t e) { return (int)(e >> 20); }
__host__ __device__ __forceinline__ int entry_level(uint32_t e) { return (int)((e >> 16) & 15u); }
__host__ __device__ __forceinline__ int entry_feature(uint32_t e) { return (int)(e & 0xffffu); }
struct ProjDev {
  int n1, n2;
  const uint8_t* valid1;
  const float* wpos1;
  const uint8_t* mpdesc1;
  const uint8_t* obs1;
  const int32_t* oct1;
  const float* xy2;
  const int32_t* oct2;
  const float* ur2;
  const uint8_t* desc2;
  float grid[6], q[4], t[3], K[4], mbf, th, scale[kProjMaxLevels];
  int forward, backward;
  int skip_behind;           // 1: points with 1/z < 0 are skipped (Frame-to-Frame overload, :1709-1712); the key-frame overload has no such test
  int max_dist;              // a candidate is viable up to this Hamming distance (TH_HIGH / ORBdist)
  int sim3_mode;             // SearchByProjection(pKF, Scw, ...): wpos1 = camera-frame points, depth z < 0 skipped, KeyFrame::IsInImage,
                             // octaves predicted - 1 ... predicted; 1: Pinhole::project, 2: invz = 1 / z, fx (x invz) + cx
  // the vpMapPoints overload (ORBmatcher.cc:43-213) instead of wpos1 / oct1 / q / t / K:
  const float* proj1;        // mTrackProjX, mTrackProjY, mTrackProjXR
  const int32_t* level1;     // mnTrackScaleLevel
  const float* viewcos1;     // mTrackViewCos
  const uint8_t* blocked2;   // feature holds an observed map point on entry (nullptr: none)
  float nnratio;
  // scratch
  uint32_t* cell_start;      // kGridCells + 1
  uint16_t* cell_items;      // n2 feature indices grouped by grid cell
  int init_taken;            // 1: the grid comes from a resident frame, the candidate kernel initialises taken_by
  int32_t* taken_by;         // n2: index of the blocker holding the feature (INT_MAX = free)
  int32_t* min_unres;        // n2
  int32_t* owner;            // n2: SearchForInitialization's vnMatches21
  float4* win;               // n1: u, v, radius, ur (= u - mbf * invzc)
  int4* rng;                 // n1: cell x range, cell y range (lo | hi << 8), minLevel, maxLevel
  unsigned long long* cand;  // n1 keys: k_fuse_search's result (best key per point)
  uint32_t* clist;           // n1 slots of kProjCand 32-bit entries (cand_entry): the points' candidate lists
  uint32_t* cref;            // n1: where a point's list starts (i * kProjCand; the resolve kernels' LDS copy: where they packed it) | entries << 26 | kRefOverflow
  uint8_t* state;            // n1: 0 unresolved, 1 resolved, 2 final this round (k_init_resolve); | kStateObs
  int32_t* choice;           // n1: best CurrentFrame feature or -1
};
constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;  // FRAME_GRID_COLS / ROWS (Frame.h:46-47)

__host__ __device__ __forceinline__ void quat_rotate(const float q[4], float px, float py, float pz, float* rx, float* ry, float* rz) {
  // Eigen QuaternionBase::_transformVector: uv = 2 (q.vec x p); p + w uv + q.vec x uv
  float ux = q[1] * pz - q[2] * py, uy = q[2] * px - q[0] * pz, uz = q[0] * py - q[1] * px;
  ux = ux + ux; uy = uy + uy; uz = uz + uz;
  const float cx = q[1] * uz - q[2] * uy, cy = q[2] * ux - q[0] * uz, cz = q[0] * uy - q[1] * ux;
  *rx = px + q[3] * ux + cx; *ry = py + q[3] * uy + cy; *rz = pz + q[3] * uz + cz;
}

// The grid cells GetFeaturesInArea(x, y, radius) walks, as ProjDev::rng holds them (lo | hi << 8); false: no cell (a NaN or
// infinite coordinate ends here as it does in the reference: the arithmetic and the order of the comparisons are its own)
__device__ __forceinline__ bool cell_window(const float grid[6], float x, float y, float radius, int* xr, int* yr) {
  const int x0 = imax(0, (int)floorf((x - grid[0] - radius) * grid[4]));
  const int x1 = imin(kGridCols - 1, (int)ceilf((x - grid[0] + radius) * grid[4]));
  const int y0 = imax(0, (int)floorf((y - grid[1] - radius) * grid[5]));
  const int y1 = imin(kGridRows - 1, (int)ceilf((y - grid[1] + radius) * grid[5]));
  if (!(x0 < kGridCols && x1 >= 0 && y0 < kGridRows && y1 >= 0)) return false;
  *xr = x0 | (x1 << 8); *yr = y0 | (y1 << 8);
  return true;
}

// the static tests of GetFeaturesInArea + the stereo check (ORBmatcher.cc:1749-1755) for feature c of a point's window
__device__ __forceinline__ bool window_accepts(const ProjDev& P, const float4& w, const int4& r, bool check_levels, int c) {
  if (check_levels) {
    const int o = P.oct2[c];
    if (o < r.z) return false;
    if (r.w >= 0 && o > r.w) return false;
  }
  const float dx = P.xy2[2 * c] - w.x, dy = P.xy2[2 * c + 1] - w.y;
  if (!(fabsf(dx) < w.z && fabsf(dy) < w.z)) return false;
  const float ur = P.ur2 ? P.ur2[c] : -1.f;  // no stereo coordinate test in the key-frame overload
  if (ur > 0 && fabsf(w.w - ur) > w.z) return false;
  return true;
}
// the same tests on values the caller has loaded (wave_candidates requests a cell's features four at a time)
__device__ __forceinline__ bool window_accepts_v(const float4& w, const int4& r, bool check_levels, int o, float x, float y, float ur) {
  if (check_levels) {
    if (o < r.z) return false;
    if (r.w >= 0 && o > r.w) return false;
  }
  const float dx = x - w.x, dy = y - w.y;
  if (!(fabsf(dx) < w.z && fabsf(dy) < w.z)) return false;
  if (ur > 0 && fabsf(w.w - ur) > w.z) return false;
  return true;
}
// visits the candidates of a point that pass those tests, in the reference's traversal order (one work-item walks the window)
template <class F>
__device__ __forceinline__ void for_candidates(const ProjDev& P, const float4& w, const int4& r, F&& f) {
  const int x0 = r.x & 0xff, x1 = r.x >> 8, y0 = r.y & 0xff, y1 = r.y >> 8;
  const bool check_levels = (r.z > 0) || (r.w >= 0);
  for (int ix = x0; ix <= x1; ++ix)
    for (int iy = y0; iy <= y1; ++iy) {
      const int cell = ix * kGridRows + iy;
      const uint32_t kb = P.cell_start[cell], ke = P.cell_start[cell + 1];
      for (uint32_t k = kb; k < ke; ++k) {
        const int c = P.cell_items[k];
        if (window_accepts(P, w, r, check_levels, c)) f(c, cell);
      }
    }
}
// The same walk by a whole WAVE (round 6: a work-item per point ran ~100 dependent gathers one after the other - 200 us for a
// frame's 2000 points): the window's cells go to the lanes in traversal order (cell t of the walk: ix = x0 + t / ny,
// iy = y0 + t % ny), 64 at a time, a lane takes its cell's features.  key_of(c, cell) is the feature's key, or ~0 when it is no
// candidate; the candidates' ranks in traversal order come from one DPP prefix sum per 64 cells and the first kProjCand keys are
// stored at their ranks: the list a single work-item would have written.  A lane keeps the first two keys of its cell in
// registers (a cell of the 64 x 48 grid holds 0.7 features of a KITTI frame on average), so the cell is walked once; a cell with
// more candidates is walked again.  Returns the number of candidates (wave-uniform).  All 64 lanes must call it.
template <class KeyOf>
__device__ __forceinline__ int wave_candidates(const ProjDev& P, const float4& w, const int4& r, unsigned long long* list, KeyOf&& key_of) {
  const int lane = lane_id();
  const int x0 = r.x & 0xff, x1 = r.x >> 8, y0 = r.y & 0xff, y1 = r.y >> 8, ny = y1 - y0 + 1, ncells = (x1 - x0 + 1) * ny;
  const bool check_levels = (r.z > 0) || (r.w >= 0);
  int base = 0;
  for (int t0 = 0; t0 < ncells; t0 += 64) {
    const int t = t0 + lane;
    uint32_t kb = 0, ke = 0;
    int cell = 0;
    if (t < ncells) {
      cell = (x0 + t / ny) * kGridRows + y0 + t % ny;
      kb = P.cell_start[cell]; ke = P.cell_start[cell + 1];
    }
    int cnt = 0;
    unsigned long long k0 = ~0ull, k1 = ~0ull;
    // four features of the cell at a time: their indices, then their positions / octaves / stereo coordinates, then the keys (the
    // descriptors) are requested back to back - device clock stamps: the walk was 12 000 of a wave's 17 000 cycles, three dependent
    // global reads per feature one feature after the other, and the lane with the fullest cell sets the wave's time
    for (uint32_t q0 = kb; q0 < ke; q0 += 4) {
      const int m = (int)(ke - q0);
      const int c0 = P.cell_items[q0], c1 = m > 1 ? (int)P.cell_items[q0 + 1] : c0, c2 = m > 2 ? (int)P.cell_items[q0 + 2] : c0,
                c3 = m > 3 ? (int)P.cell_items[q0 + 3] : c0;
      const int cs[4] = {c0, c1, c2, c3};
      float fx[4], fy[4], fu[4];
      int fo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        fx[j] = P.xy2[2 * cs[j]]; fy[j] = P.xy2[2 * cs[j] + 1];
        fo[j] = check_levels ? P.oct2[cs[j]] : 0;
        fu[j] = P.ur2 ? P.ur2[cs[j]] : -1.f;
      }
      unsigned long long keys[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        keys[j] = (j < m && window_accepts_v(w, r, check_levels, fo[j], fx[j], fy[j], fu[j])) ? key_of(cs[j], cell) : ~0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (keys[j] != ~0ull) {
          if (cnt == 0) k0 = keys[j]; else if (cnt == 1) k1 = keys[j];
          ++cnt;
        }
    }
    const int incl = wave_inclusive_scan(cnt);
    int pos = base + incl - cnt;
    base += __shfl(incl, 63);
    if (cnt > 0 && pos < kProjCand) {
      if (cnt <= 2) {
        list[pos] = k0;
        if (cnt == 2 && pos + 1 < kProjCand) list[pos + 1] = k1;
      } else {
        for (uint32_t k = kb; k < ke && pos < kProjCand; ++k) {
          const int c = P.cell_items[k];
          const unsigned long long key = window_accepts(P, w, r, check_levels, c) ? key_of(c, cell) : ~0ull;
          if (key != ~0ull) list[pos++] = key;
        }
      }
    }
  }
  return base;
}
__device__ __forceinline__ unsigned long long proj_key(int dist, int cell, int c) {
  // strict '<' over the traversal (cells x-major, feature index inside a cell) == minimum of this key
  return ((unsigned long long)dist << 32) | ((unsigned long long)cell << 16) | (unsigned)c;
}

// The wave that walked a point's window hands its list to the resolve kernel (round 6: the resolve rounds were chains of dependent
// global reads of 8-byte keys - ~8 us per round for a frame's 2000 points).  The keys the walk left in the wave's LDS slots
// (traversal order) become 32-bit entries in the point's 16-entry slot of P.clist, 64 bytes the resolve kernel fetches with four
// independent 16-byte loads per point and packs into LDS: its rounds never touch global memory.  (A dense list reserved with one
// atomic per wave was tried first: ~3000 returning atomics on one address cost the candidate kernels 10 - 20 us.)
// `sorted`: the entries are written in ascending key order (best-only searches: a point's choice is then the first entry still
// available).  All 64 lanes call it; returns the point's cref word (wave-uniform).
template <class Enc>
__device__ __forceinline__ uint32_t publish_candidates(const ProjDev& P, int i, const unsigned long long* keys, int total, bool sorted, Enc&& enc) {
  wave_sync();
  const int lane = lane_id();
  if (total > kProjCand) return kRefOverflow;
  const int n = total;
  const unsigned long long key = lane < n ? keys[lane] : ~0ull;
  int rank = lane;
  if (sorted) {
    rank = 0;
    for (int j = 0; j < n; ++j) rank += keys[j] < key ? 1 : 0;
  }
  const uint32_t start = (uint32_t)i * kProjCand;
  if (lane < n) P.clist[start + rank] = enc(key);
  return start | ((uint32_t)n << 26);
}
// what the candidate kernels leave in P.state: 0 = unresolved, 1 = resolved | kStateObs: the point blocks the feature it takes
constexpr uint8_t kStateObs = 0x80;

// grid = 1, block = kGridBS.  LDS = true (frames of up to kGridLdsN2 features): a feature's cell is computed once and kept in
// LDS, the cells' item lists are built and put in ascending order there and leave with one coalesced pass - the first form ran
// count, scatter and the per-cell ordering as chains of dependent global reads (20 us for a frame's 2000 features, round 6).
constexpr int kGridBS = 1024, kGridLdsN2 = 8192;
template <bool LDS>
__global__ __launch_bounds__(kGridBS) void k_proj_grid(ProjDev P) {
  __shared__ uint32_t s_fill[kGridCells], s_start[LDS ? kGridCells : 1];
  __shared__ uint32_t s_scan[kGridBS / 64 + 1];
  __shared__ uint16_t s_cell[LDS ? kGridLdsN2 : 1], s_items[LDS ? kGridLdsN2 : 1];
  const int tid = threadIdx.x;
  auto cell_of = [&](int c) {
    const int px = (int)roundf((P.xy2[2 * c] - P.grid[0]) * P.grid[4]), py = (int)roundf((P.xy2[2 * c + 1] - P.grid[1]) * P.grid[5]);
    return (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) ? px * kGridRows + py : -1;
  };
  for (int c = tid; c < kGridCells; c += kGridBS) s_fill[c] = 0;
  __syncthreads();
  for (int c = tid; c < P.n2; c += kGridBS) {
    const int cell = cell_of(c);
    if (LDS) s_cell[c] = (uint16_t)cell;   // 0xffff: outside the grid
    if (cell >= 0) atomicAdd(&s_fill[cell], 1u);
    P.taken_by[c] = (P.blocked2 && P.blocked2[c]) ? -1 : INT_MAX;  // -1: held by a point from before the call
  }
  __syncthreads();
  // a work-item owns three consecutive cells: ONE workgroup prefix sum for the 3072 cells (three chunks of 1024 took three)
  static_assert(kGridCells == 3 * kGridBS, "three cells per work-item");
  uint32_t carry;
  {
    const uint32_t v0 = s_fill[3 * tid], v1 = s_fill[3 * tid + 1], v2 = s_fill[3 * tid + 2];
    const uint32_t ex = block_exclusive_scan<uint32_t>(v0 + v1 + v2, s_scan, &carry);
    const uint32_t st[3] = {ex, ex + v0, ex + v0 + v1};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      P.cell_start[3 * tid + q] = st[q]; s_fill[3 * tid + q] = st[q];
      if (LDS) s_start[3 * tid + q] = st[q];
    }
  }
  if (tid == 0) P.cell_start[kGridCells] = carry;
  __syncthreads();
  uint16_t* items = LDS ? s_items : P.cell_items;
  for (int c = tid; c < P.n2; c += kGridBS) {
    const int cell = LDS ? (s_cell[c] == 0xffffu ? -1 : (int)s_cell[c]) : cell_of(c);
    if (cell >= 0) items[atomicAdd(&s_fill[cell], 1u)] = (uint16_t)c;
  }
  __syncthreads();
  // ascending feature index inside every cell = the push_back order of AssignFeaturesToGrid (cells hold a handful of items)
  for (int cell = tid; cell < kGridCells; cell += kGridBS) {
    const uint32_t b = LDS ? s_start[cell] : P.cell_start[cell], e = s_fill[cell];
    for (uint32_t i = b + 1; i < e; ++i) {
      const uint16_t v = items[i];
      uint32_t j = i;
      while (j > b && items[j - 1] > v) { items[j] = items[j - 1]; --j; }
      items[j] = v;
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = tid; k < carry; k += kGridBS) P.cell_items[k] = s_items[k];
  }
}
static void launch_proj_grid(const ProjDev& P, hipStream_t s) {
  if (P.n2 <= kGridLdsN2) hipLaunchKernelGGL(k_proj_grid<true>, dim3(1), dim3(kGridBS), 0, s, P);
  else hipLaunchKernelGGL(k_proj_grid<false>, dim3(1), dim3(kGridBS), 0, s, P);
}

// With the grid taken from a resident frame nobody runs k_proj_grid: its other job - who holds a feature before the call - is
// done by the candidate kernels' workgroups on the way (the resolve kernel behind them is the first reader).
__device__ __forceinline__ void init_taken_by(const ProjDev& P) {
  if (!P.init_taken) return;
  for (int c = (int)(blockIdx.x * blockDim.x + threadIdx.x); c < P.n2; c += (int)(gridDim.x * blockDim.x))
    P.taken_by[c] = (P.blocked2 && P.blocked2[c]) ? -1 : INT_MAX;
}

// The frame of the three candidate kernels (grid = ceil(n1 / 4), block = 256 = one wave per point, wave_point() names it): what a
// point leaves for its resolve kernel, collected by collect_candidates when it has a window and stored by store_candidates
constexpr int kPointsPerBlock = 4;
__device__ __forceinline__ int wave_point() { return blockIdx.x * kPointsPerBlock + wave_id(); }
struct CandResult { uint32_t ref = 0; uint8_t st = 1; };   // no window: an empty list, resolved
// walk, window, list: key_of / keys as for wave_candidates, sorted / enc as for publish_candidates.  All 64 lanes call it.
template <class KeyOf, class Enc>
__device__ __forceinline__ CandResult collect_candidates(const ProjDev& P, int i, const float4& w, const int4& r, unsigned long long* keys,
                                                         bool sorted, KeyOf&& key_of, Enc&& enc) {
  CandResult res;
  const int total = wave_candidates(P, w, r, keys, key_of);
  if (lane_id() == 0) { P.win[i] = w; P.rng[i] = r; }
  res.ref = publish_candidates(P, i, keys, total, sorted, enc);
  res.st = total > 0 ? 0 : 1;  // no viable candidate: no match whatever the others do
  return res;
}
// blockers: the search has points that block the feature they take (P.obs1)
__device__ __forceinline__ void store_candidates(const ProjDev& P, int i, const CandResult& res, bool blockers) {
  if (lane_id() == 0) { P.choice[i] = -1; P.cref[i] = res.ref; P.state[i] = res.st | ((blockers && P.obs1[i]) ? kStateObs : 0); }
}

// one wave per LastFrame map point: projection and search window (ORBmatcher.cc:1696-1735, computed by every lane alike), then
// its viable candidates by wave_candidates
__global__ __launch_bounds__(256) void k_proj_candidates(ProjDev P) {
  __shared__ unsigned long long s_keys[kPointsPerBlock][kProjCand];
  init_taken_by(P);
  const int i = wave_point();
  if (i >= P.n1) return;
  CandResult res;
  // everything the point needs is requested up front (it was four dependent global reads: valid -> position -> octave -> descriptor)
  const uint8_t valid = P.valid1[i];
  const float wx = P.wpos1[3 * i], wy = P.wpos1[3 * i + 1], wz = P.wpos1[3 * i + 2];
  const int oct_i = P.oct1[i];
  const Desc256 d = load_desc(P.mpdesc1, i);
  if (valid) {
    float x, y, z;
    if (P.sim3_mode) {
      x = wx; y = wy; z = wz;
    } else {
      quat_rotate(P.q, wx, wy, wz, &x, &y, &z);
      x += P.t[0]; y += P.t[1]; z += P.t[2];
    }
    const float invzc = (float)(1.0 / (double)z);
    float u, v;
    if (P.sim3_mode == 2) {
      const float invz = __fdiv_rn(1.0f, z);
      u = P.K[0] * (x * invz) + P.K[2]; v = P.K[1] * (y * invz) + P.K[3];
    } else {
      u = __fdiv_rn(P.K[0] * x, z) + P.K[2]; v = __fdiv_rn(P.K[1] * y, z) + P.K[3];
    }
    // NaN / inf coordinates never produce candidates in the reference either (empty cell range)
    const bool in_view = P.sim3_mode ? (!(z < 0.0f) && u >= P.grid[0] && u < P.grid[2] && v >= P.grid[1] && v < P.grid[3])
                                     : (!(P.skip_behind && invzc < 0) && u == u && v == v && !(u < P.grid[0] || u > P.grid[2]) &&
                                        !(v < P.grid[1] || v > P.grid[3]));
    if (in_view) {
      const int oct = oct_i;
      const float radius = P.th * P.scale[oct];
      int4 r;
      if (P.sim3_mode) { r.z = oct - 1; r.w = oct; }
      else if (P.forward) { r.z = oct; r.w = -1; }
      else if (P.backward) { r.z = 0; r.w = oct; }
      else { r.z = oct - 1; r.w = oct + 1; }
      if (cell_window(P.grid, u, v, radius, &r.x, &r.y)) {
        const float4 w = make_float4(u, v, radius, u - P.mbf * invzc);
        res = collect_candidates(P, i, w, r, s_keys[wave_id()], true, [&](int c, int cell) {
          const int dist = desc_dist(d, P.desc2, c);
          return dist <= P.max_dist ? proj_key(dist, cell, c) : ~0ull;   // bestDist > TH_HIGH: not viable
        }, [](unsigned long long key) { return cand_entry((int)(key >> 32), 0, (int)(key & 0xffffu)); });
      }
    }
  }
  store_candidates(P, i, res, true);
}

// the feature point i takes among those not held by a lower-index blocker: the smallest key (-1 = none)
__device__ __forceinline__ int proj_best(const ProjDev& P, const int32_t* taken_by, const uint32_t* cref, const uint32_t* clist, int i) {
  const uint32_t r = cref[i];
  if (!(r & kRefOverflow)) {
    const uint32_t* e = clist + ref_start(r);
    for (int k = 0, n = ref_n(r); k < n; ++k) {   // ascending keys
      const int c = entry_feature(e[k]);
      if (taken_by[c] >= i) return c;
    }
    return -1;
  }
  unsigned long long best = ~0ull;
  const Desc256 d = load_desc(P.mpdesc1, i);
  for_candidates(P, P.win[i], P.rng[i], [&](int c, int cell) {
    if (taken_by[c] < i) return;
    const int dist = desc_dist(d, P.desc2, c);
    if (dist > P.max_dist) return;
    const unsigned long long key = proj_key(dist, cell, c);
    if (key < best) best = key;
  });
  return best == ~0ull ? -1 : (int)(best & 0xffffu);
}

// The resolve kernels' view of the lists: packed into LDS when the call's points (cref) and entries fit, else where the candidate kernels left them
constexpr int kResolveLdsN2 = 6144, kResolveLdsN1 = 8192, kResolveLdsList = 12288;
constexpr int kUCap = 4096;   // unresolved points a round can hand to the next one as a list (resolve_rounds)
constexpr int kResolveBS = 1024;
struct ListView { const uint32_t* cref; const uint32_t* clist; };
// (the copies of taken_by and state ride in the same trips: three independent loads per trip instead of three loops of dependent ones)
template <bool LDS>
__device__ __forceinline__ ListView stage_lists(const ProjDev& P, int32_t* s_taken, uint8_t* s_state, uint32_t* s_ref, uint32_t* s_list, int* s_total) {
  ListView v{P.cref, P.clist};
  if (LDS) {
    const int tid = threadIdx.x, lane = lane_id();
    if (tid == 0) *s_total = 0;
    __syncthreads();
    // where a point's entries go: any packing will do, so a wave's points take one range (one LDS atomic per wave and trip)
    for (int i0 = 0; i0 < P.n1 || i0 < P.n2; i0 += kResolveBS) {
      const int i = i0 + tid;
      const uint32_t r = i < P.n1 ? P.cref[i] : 0u;
      const uint8_t st = i < P.n1 ? P.state[i] : (uint8_t)0;
      const int32_t tk = i < P.n2 ? P.taken_by[i] : 0;
      if (i < P.n1) s_state[i] = st;
      if (i < P.n2) s_taken[i] = tk;
      const int n = (r & kRefOverflow) ? 0 : ref_n(r);
      const int incl = wave_inclusive_scan(n), tot = __shfl(incl, 63);
      int base = 0;
      if (lane == 0 && tot > 0) base = atomicAdd(s_total, tot);
      base = __shfl(base, 0);
      if (i < P.n1) s_ref[i] = (r & kRefOverflow) | ((uint32_t)n << 26) | (uint32_t)(base + incl - n);
    }
    __syncthreads();
    if (*s_total <= kResolveLdsList) {
      for (int i = tid; i < P.n1; i += kResolveBS) {
        const uint32_t r = s_ref[i];
        const int n = ref_n(r);
        if (n == 0) continue;
        const uint4* src = reinterpret_cast<const uint4*>(P.clist + (size_t)i * kProjCand);
        const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
        const uint32_t e[kProjCand] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
        uint32_t* dst = s_list + ref_start(r);
#pragma unroll
        for (int k = 0; k < kProjCand; ++k)
          if (k < n) dst[k] = e[k];
      }
      v.clist = s_list;
    } else {
      for (int i = tid; i < P.n1; i += kResolveBS) s_ref[i] = P.cref[i];
    }
    v.cref = s_ref;
  }
  return v;
}

// grid = 1, block = kResolveBS.  LDS = true (frames of up to kResolveLdsN2 features, kResolveLdsN1 points: every KITTI-size call):
// who holds a feature, the lowest unresolved blocker per feature and the points' states live in LDS for the whole kernel - a
// round is three passes over them, and with the arrays in global memory every pass was a chain of dependent ~1 us loads
// (round 6: 8 rounds of 17 us for a frame's 2000 points).
// min_unres[c] = (stamp << 20 | lowest unresolved blocker that may still take c), stamp = kStampMax - round: a round's entries are
// smaller than everything older rounds left behind, so the array is not cleared between rounds (one pass and one barrier per
// round less); it is refilled with INT_MAX every kStampMax rounds (the worst case - a chain of n1 blockers - takes n1 rounds).
constexpr int kStampMax = 2047;
__device__ __forceinline__ bool lower_unresolved(int m, int stamp, int i) { return (m >> 20) == stamp && (m & 0xfffff) < i; }
// The round loop of the three resolve kernels.  announce(i, stamp): point i, if it is an unresolved blocker, publishes itself on what it
// may still take; decide(i, stamp): point i becomes final (and commits) or not - true while it stays unresolved.  Rounds: all points;
// from the second round on the LIST of the points the round before left unresolved (up to kUCap of them) - a wave runs a point's chain
// of dependent LDS accesses as soon as ONE of its lanes holds an unresolved point, and the few dozen points of the late rounds,
// scattered over all waves, cost every wave its full time; and once at most 64 are left, ONE wave finishes them with wave-level
// synchronisation only: what is left then is a chain of points waiting for each other, one short round per link (a KITTI frame: ~10
// rounds, 3.5 us each while all 16 waves and three workgroup barriers took part in every one).
template <bool LDS, class Announce, class Decide>
__device__ __forceinline__ void resolve_rounds(int n1, int n2, int32_t* min_unres, int* s_unres, uint16_t (*s_ulist)[LDS ? kUCap : 1],
                                               Announce&& announce, Decide&& decide) {
  const int tid = threadIdx.x;
  if (tid < 2) s_unres[tid] = 0;
  bool use_list = false;
  int n_walk = n1;   // points this round looks at: all, or the entries of s_ulist[b ^ 1]
  int round = 0, left = 0;
  for (; round <= n1; ++round) {
    const int stamp = kStampMax - round % kStampMax, b = round & 1;
    if (round % kStampMax == 0) {
      __syncthreads();
      for (int c = tid; c < n2; c += kResolveBS) min_unres[c] = INT_MAX;
    }
    __syncthreads();
    for (int t = tid; t < n_walk; t += kResolveBS) announce(use_list ? (int)s_ulist[b ^ 1][t] : t, stamp);
    __syncthreads();
    for (int t = tid; t < n_walk; t += kResolveBS) {
      const int i = use_list ? (int)s_ulist[b ^ 1][t] : t;
      if (decide(i, stamp)) {   // counted, and listed for the next round
        const int pos = atomicAdd(&s_unres[b], 1);
        if (LDS && pos < kUCap) s_ulist[b][pos] = (uint16_t)i;
      }
    }
    if (tid == 0) s_unres[b ^ 1] = 0;
    __syncthreads();
    left = s_unres[b];
    if (left == 0) return;
    if (LDS && left <= 64) break;
    use_list = LDS && left <= kUCap;
    n_walk = use_list ? left : n1;
  }
  if (!LDS || wave_id() != 0) return;
  const int lane = lane_id();
  int mine = lane < left ? (int)s_ulist[round & 1][lane] : -1;
  for (++round; round <= n1 + 1; ++round) {
    const int stamp = kStampMax - round % kStampMax;
    if (round % kStampMax == 0) {
      wave_sync();
      for (int c = lane; c < n2; c += 64) min_unres[c] = INT_MAX;
    }
    wave_sync();
    if (mine >= 0) announce(mine, stamp);
    wave_sync();
    if (mine >= 0 && !decide(mine, stamp)) mine = -1;
    wave_sync();
    if (__ballot(mine >= 0) == 0ull) break;
  }
}

// What a resolve kernel keeps in LDS, declared ONCE per kernel as `__shared__`.  LDS = false: the round counters only, everything
// else stays where the candidate kernels left it.  LDS = true: members in descending alignment, so no padding - the kernels sit
// 8 KB below what a workgroup can have.
template <bool LDS>
struct ResolveShared { int s_unres[2]; };
template <>
struct ResolveShared<true> {
  int s_unres[2], s_total;
  int32_t s_taken[kResolveLdsN2], s_min[kResolveLdsN2];
  uint32_t s_ref[kResolveLdsN1], s_list[kResolveLdsList];
  uint16_t s_ulist[2][kUCap];
  uint8_t s_state[kResolveLdsN1];
};
static_assert(sizeof(ResolveShared<true>) == 12 + 8 * kResolveLdsN2 + 5 * kResolveLdsN1 + 4 * kResolveLdsList + 4 * kUCap, "padding in the resolve kernels' LDS");
// what a search's announce / decide see of the call: who holds a feature, the lowest unresolved blocker per feature, the points'
// states (LDS or global memory) and the candidate lists
struct ResolveView {
  int32_t* taken_by;
  int32_t* min_unres;
  uint8_t* state;
  ListView L;
};
// The body of a resolve kernel: stages the call's arrays, then runs the rounds with the search's two rules - announce(R, i, stamp)
// and decide(R, i, stamp), see resolve_rounds.  With LDS the rounds are instantiated twice, for the lists in LDS and for the lists
// where the candidate kernel left them: with ONE pointer chosen at run time the entries were read with flat loads.
template <bool LDS, class Announce, class Decide>
__device__ __forceinline__ void resolve_run(const ProjDev& P, ResolveShared<LDS>& sh, Announce&& announce, Decide&& decide) {
  auto run = [&](const ResolveView R, uint16_t (*ulist)[LDS ? kUCap : 1]) {
    resolve_rounds<LDS>(P.n1, P.n2, R.min_unres, sh.s_unres, ulist, [&](int i, int stamp) { announce(R, i, stamp); },
                        [&](int i, int stamp) { return decide(R, i, stamp); });
  };
  if constexpr (LDS) {
    const ListView staged = stage_lists<true>(P, sh.s_taken, sh.s_state, sh.s_ref, sh.s_list, &sh.s_total);
    if (staged.clist != P.clist) run(ResolveView{sh.s_taken, sh.s_min, sh.s_state, ListView{sh.s_ref, sh.s_list}}, sh.s_ulist);
    else run(ResolveView{sh.s_taken, sh.s_min, sh.s_state, ListView{sh.s_ref, P.clist}}, sh.s_ulist);
  } else {
    run(ResolveView{P.taken_by, P.min_unres, P.state, ListView{P.cref, P.clist}}, nullptr);   // no list of the unresolved without LDS
  }
}

template <bool LDS>
__global__ __launch_bounds__(kResolveBS) void k_proj_resolve(ProjDev P) {
  __shared__ ResolveShared<LDS> sh;
  resolve_run<LDS>(P, sh,
    // every unresolved blocker announces itself on the features it may still take
    [&](const ResolveView& R, int i, int stamp) {
      if (R.state[i] != kStateObs) return;   // unresolved and a blocker
      const uint32_t r = R.L.cref[i];
      const int me = (stamp << 20) | i;
      if (!(r & kRefOverflow)) {
        const uint32_t* e = R.L.clist + ref_start(r);
        for (int k = 0, n = ref_n(r); k < n; ++k) {
          const int c = entry_feature(e[k]);
          if (R.taken_by[c] >= i) atomicMin(&R.min_unres[c], me);
        }
      } else {
        const Desc256 d = load_desc(P.mpdesc1, i);
        for_candidates(P, P.win[i], P.rng[i], [&](int c, int) {
          if (R.taken_by[c] < i) return;
          if (desc_dist(d, P.desc2, c) <= P.max_dist) atomicMin(&R.min_unres[c], me);
        });
      }
    },
    // decide AND commit in one pass: a point whose best available feature no lower unresolved blocker can still take is final
    // and occupies it at once.  What a concurrent work-item sees of that store does not matter: a HIGHER point that misses it
    // picks the same feature, finds this point's announcement in front of it and waits a round; one that sees it takes its next
    // choice, which is what the sequential loop would have given it; LOWER points never want a feature that becomes final here
    // (their announcement would have held this point back).  Two blockers never become final on one feature in the same round.
    [&](const ResolveView& R, int i, int stamp) {
      const uint8_t st = R.state[i];
      if (st & 0x7f) return false;
      const int c = proj_best(P, R.taken_by, R.L.cref, R.L.clist, i);
      if (c < 0) { R.state[i] = st | 1; P.choice[i] = -1; return false; }   // everything viable is taken: no match
      if (lower_unresolved(R.min_unres[c], stamp, i)) return true;          // somebody in front of i can still take c
      R.state[i] = st | 1; P.choice[i] = c;
      if (st & kStateObs) R.taken_by[c] = i;
      return false;
    });
}

// ------------------------------------------------------------------------------------------------
// The search of ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false)
// (/root/reference/src/ORBmatcher.cc:1148-1338, single camera) with KeyFrame::GetFeaturesInArea / IsInImage
// (src/KeyFrame.cc:704-753): every map point looks for its best feature on its own - what the loop does with a match
// (Replace / AddObservation / AddMapPoint) changes MapPoint and KeyFrame objects and stays with the caller.
// Uses ProjDev: wpos1, mpdesc1, oct1 (= predicted level), valid1, the grid of k_proj_grid, q / t / K, mbf, th, scale;
// cand[i] receives the best (distance, cell order, feature) key or ~0.
struct FuseDev {
  float inv_sigma2[kProjMaxLevels];
  int cam_frame;  // 1: wpos1 already holds camera-frame coordinates (the caller applied its SE3 / Sim3)
  int proj_form;  // 0: Pinhole::project, fx x / z + cx; 1: invz = (float)(1.0 / z), fx (x invz) + cx (SearchBySim3, :1508-1513)
  int chi2_gate;  // 1: the reprojection-error gates of Fuse(pKF, vpMapPoints, th)
};

// grid = ceil(n1 / 4), block = 256 = one wave per map point (round 6; a work-item per point walked ~100 dependent gathers: 30 us
// for 2500 points): the window's cells go to the lanes in traversal order, a lane keeps the smallest (distance, cell, feature)
// key of its cells - the cell number grows along the traversal, so the smallest key IS the reference's first minimum - and the
// wave's minimum over (distance, cell) names the one lane that holds it.
__global__ __launch_bounds__(256) void k_fuse_search(ProjDev P, FuseDev Fz) {
  const int i = wave_point();
  if (i >= P.n1) return;
  const int lane = lane_id();
  unsigned long long best = ~0ull;
  if (P.valid1[i]) {
    float x, y, z;
    if (Fz.cam_frame) {
      x = P.wpos1[3 * i]; y = P.wpos1[3 * i + 1]; z = P.wpos1[3 * i + 2];
    } else {
      quat_rotate(P.q, P.wpos1[3 * i], P.wpos1[3 * i + 1], P.wpos1[3 * i + 2], &x, &y, &z);
      x += P.t[0]; y += P.t[1]; z += P.t[2];
    }
    if (!(z < 0.0f)) {  // depth must be positive (:1201-1206)
      const float invz = Fz.proj_form == 1 ? (float)(1.0 / (double)z) : __fdiv_rn(1.0f, z);
      float u, v;
      if (Fz.proj_form == 1) { u = P.K[0] * (x * invz) + P.K[2]; v = P.K[1] * (y * invz) + P.K[3]; }
      else { u = __fdiv_rn(P.K[0] * x, z) + P.K[2]; v = __fdiv_rn(P.K[1] * y, z) + P.K[3]; }
      if (u >= P.grid[0] && u < P.grid[2] && v >= P.grid[1] && v < P.grid[3]) {  // KeyFrame::IsInImage
        const float ur = u - P.mbf * invz;
        const int level = P.oct1[i];
        const float radius = P.th * P.scale[level];
        int xr, yr;
        if (cell_window(P.grid, u, v, radius, &xr, &yr)) {
          const Desc256 d = load_desc(P.mpdesc1, i);
          const int x0 = xr & 0xff, x1 = xr >> 8, y0 = yr & 0xff, y1 = yr >> 8, ny = y1 - y0 + 1, ncells = (x1 - x0 + 1) * ny;
          for (int t = lane; t < ncells; t += 64) {
            const int cell = (x0 + t / ny) * kGridRows + y0 + t % ny;
            const uint32_t kb = P.cell_start[cell], ke = P.cell_start[cell + 1];
            for (uint32_t k = kb; k < ke; ++k) {
              const int c = P.cell_items[k];
              const float kpx = P.xy2[2 * c], kpy = P.xy2[2 * c + 1];
              if (!(fabsf(kpx - u) < radius && fabsf(kpy - v) < radius)) continue;
              const int kl = P.oct2[c];
              if (kl < level - 1 || kl > level) continue;
              // reprojection error gate, chi-square at 95 % with 3 / 2 degrees of freedom (:1262-1288)
              const float ex = u - kpx, ey = v - kpy;
              const float kpr = P.ur2 ? P.ur2[c] : -1.f;
              if (!Fz.chi2_gate) {
              } else if (kpr >= 0) {
                const float er = ur - kpr;
                const float e2 = ex * ex + ey * ey + er * er;
                if ((double)(e2 * Fz.inv_sigma2[kl]) > 7.8) continue;
              } else {
                const float e2 = ex * ex + ey * ey;
                if ((double)(e2 * Fz.inv_sigma2[kl]) > 5.99) continue;
              }
              const int dist = desc_dist(d, P.desc2, c);
              const unsigned long long key = proj_key(dist, cell, c);
              if (key < best) best = key;  // strict '<' over the traversal order
            }
          }
        }
      }
    }
  }
  // (distance << 16 | cell) of the wave's smallest key: a cell belongs to one lane, so exactly one lane matches - or all do, with ~0
  const uint32_t m = wave_min_uniform((uint32_t)(best >> 16));
  if ((uint32_t)(best >> 16) == m && (best != ~0ull || lane == 0)) P.cand[i] = best;
}

// ------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, ...) (ORBmatcher.cc:43-213; single camera),
// the matcher of Tracking::SearchLocalPoints.  Same greedy order and blocking rule as above, but a point's decision is
// best AND second-best distance with their pyramid levels (ratio test only inside one level), so the candidates are
// kept in traversal order (distance << 32 | level << 16 | feature) and the sequential scan is replayed on the available
// ones; a point is final once no unresolved lower-index blocker can still take ANY of its available candidates.
struct LocalScan {
  int best_dist = 256, best_level = -1, best_dist2 = 256, best_level2 = -1, best_idx = -1;
  __device__ __forceinline__ void visit(int dist, int level, int c) {  // ORBmatcher.cc:104-122
    if (dist < best_dist) { best_dist2 = best_dist; best_dist = dist; best_level2 = best_level; best_level = level; best_idx = c; }
    else if (dist < best_dist2) { best_level2 = level; best_dist2 = dist; }
  }
  __device__ __forceinline__ int accept(float nnratio) const {  // ORBmatcher.cc:125-141; feature index or -1
    if (best_dist > 100 /* TH_HIGH */) return -1;
    if (best_level == best_level2 && (float)best_dist > nnratio * (float)best_dist2) return -1;
    return best_idx;
  }
};

// one wave per map point (the candidate kernels' frame: wave_point)
__global__ __launch_bounds__(256) void k_local_candidates(ProjDev P) {
  __shared__ unsigned long long s_keys[kPointsPerBlock][kProjCand];
  init_taken_by(P);
  const int i = wave_point();
  if (i >= P.n1) return;
  CandResult res;
  // (requested up front, as in k_proj_candidates)
  const uint8_t valid = P.valid1[i];
  const int level_i = P.level1[i];
  const float viewcos = P.viewcos1[i], px = P.proj1[3 * i], py = P.proj1[3 * i + 1], pxr = P.proj1[3 * i + 2];
  const Desc256 d = load_desc(P.mpdesc1, i);
  if (valid) {
    const int level = level_i;
    float r = (double)viewcos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos: the literal is a double in the reference
    if (P.th != 1.0f) r *= P.th;
    const float x = px, y = py;
    const float radius = r * P.scale[level];
    int4 rg = make_int4(0, 0, level - 1, level);
    if (x == x && y == y && cell_window(P.grid, x, y, radius, &rg.x, &rg.y)) {
      const float4 w = make_float4(x, y, radius, pxr);
      res = collect_candidates(P, i, w, rg, s_keys[wave_id()], false /* traversal order: the scan is replayed */, [&](int c, int) {
        return ((unsigned long long)desc_dist(d, P.desc2, c) << 32) | ((unsigned long long)P.oct2[c] << 16) | (unsigned)c;
      }, [](unsigned long long key) { return cand_entry((int)(key >> 32), (int)((key >> 16) & 0xffffu), (int)(key & 0xffffu)); });
    }
  }
  store_candidates(P, i, res, true);
}

// visits the candidates of point i that no lower-index blocker holds, in traversal order: f(dist, level, c)
template <class F>
__device__ __forceinline__ void local_available(const ProjDev& P, const int32_t* taken_by, const ListView& L, int i, F&& f) {
  const uint32_t r = L.cref[i];
  if (!(r & kRefOverflow)) {
    const uint32_t* e = L.clist + ref_start(r);
    for (int k = 0, n = ref_n(r); k < n; ++k) {
      const int c = entry_feature(e[k]);
      if (taken_by[c] >= i) f(entry_dist(e[k]), entry_level(e[k]), c);
    }
    return;
  }
  const Desc256 d = load_desc(P.mpdesc1, i);
  for_candidates(P, P.win[i], P.rng[i], [&](int c, int) {
    if (taken_by[c] < i) return;
    f(desc_dist(d, P.desc2, c), P.oct2[c], c);
  });
}

// grid = 1, block = kResolveBS; LDS, round stamps and the merged decide + commit pass as for k_proj_resolve
template <bool LDS>
__global__ __launch_bounds__(kResolveBS) void k_local_resolve(ProjDev P) {
  __shared__ ResolveShared<LDS> sh;
  resolve_run<LDS>(P, sh,
    [&](const ResolveView& R, int i, int stamp) {
      if (R.state[i] != kStateObs) return;   // unresolved and a blocker
      const int me = (stamp << 20) | i;
      local_available(P, R.taken_by, R.L, i, [&](int dist, int, int c) { if (dist <= 100) atomicMin(&R.min_unres[c], me); });
    },
    // (a settled point's available candidates carry no announcement of a lower point, so no lower point can occupy one of them in
    // this pass; a higher point's store leaves taken_by[c] >= i: still available to i)
    [&](const ResolveView& R, int i, int stamp) {
      const uint8_t st = R.state[i];
      if (st & 0x7f) return false;
      LocalScan sc;
      bool settled = true;
      local_available(P, R.taken_by, R.L, i, [&](int dist, int level, int c) {
        sc.visit(dist, level, c);
        if (lower_unresolved(R.min_unres[c], stamp, i)) settled = false;  // somebody in front of i may still take this feature
      });
      if (!settled) return true;
      const int c = sc.accept(P.nnratio);
      R.state[i] = st | 1; P.choice[i] = c;
      if (c >= 0 && (st & kStateObs)) R.taken_by[c] = i;
      return false;
    });
}

// ------------------------------------------------------------------------------------------------
// bool Frame::isInFrustum(MapPoint*, float viewingCosLimit) (src/Frame.cc:602-664, Nleft == -1) with MapPoint::PredictScale
// (src/MapPoint.cc:531-546) and Pinhole::project (src/CameraModels/Pinhole.cpp:43-49): the loop Tracking::SearchLocalPoints
// (src/Tracking.cc:3399-3420) runs in front of the matcher above.  Every point on its own, fp32 in the reference's order (the
// three Eigen reductions: frustum_math.h), `/` and sqrt correctly rounded, logf as glibc evaluates it (logf_glibc.h).
// The comparisons are written in the reference's sense, so a NaN or infinite projection passes and fails what it does there.
struct FrustumDev {
  int n1;
  // map points: index j = slot1 ? slot1[i] : i into the five arrays (the call's staged arrays, or a pool's)
  const uint8_t* consider1;
  const int32_t* slot1;
  const float* wpos; const float* normal; const float* min_dist; const float* max_dist;
  const uint8_t* desc;         // read only with slot1: a considered point's descriptor is copied to mpdesc1[i]
  float Rcw[9], tcw[3], Ow[3], K[4], bounds[4], mbf, log_scale, cos_limit, th_far;
  int far_points, n_levels;
  // results
  uint8_t* in_view;
  rgbl_frustum_record* rec;
  // what k_local_candidates reads (ProjDev::valid1, proj1, level1, viewcos1, mpdesc1); nullptr for the cull alone
  uint8_t* valid1; float* proj1; int32_t* level1; float* viewcos1; uint8_t* mpdesc1;
};

// grid = ceil(n1 / 256), block = 256: one work-item per map point
__global__ __launch_bounds__(256) void k_frustum(FrustumDev F) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= F.n1) return;
  uint8_t in_view = 0;
  rgbl_frustum_record r;
  r.proj_x = -1.f; r.proj_y = -1.f;               // Frame.cc:605-607
  r.proj_xr = 0.f; r.depth = 0.f; r.view_cos = 0.f; r.level = 0;
  if (!F.consider1 || F.consider1[i]) {
    const int j = F.slot1 ? F.slot1[i] : i;
    if (F.mpdesc1 && F.slot1) {
      const uint4* src = reinterpret_cast<const uint4*>(F.desc + (size_t)j * 32);
      uint4* dst = reinterpret_cast<uint4*>(F.mpdesc1 + (size_t)i * 32);
      const uint4 a = src[0], b = src[1];
      dst[0] = a; dst[1] = b;
    }
    const float p0 = F.wpos[3 * j], p1 = F.wpos[3 * j + 1], p2 = F.wpos[3 * j + 2];
    const float x = fr_row_times(F.Rcw, p0, p1, p2) + F.tcw[0], y = fr_row_times(F.Rcw + 3, p0, p1, p2) + F.tcw[1],
                z = fr_row_times(F.Rcw + 6, p0, p1, p2) + F.tcw[2];
    const float pc_dist = fr_norm(x, y, z);
    const float invz = __fdiv_rn(1.0f, z);
    do {
      if (z < 0.0f) break;                          // :619 (a zero depth goes on)
      const float u = __fdiv_rn(F.K[0] * x, z) + F.K[2], v = __fdiv_rn(F.K[1] * y, z) + F.K[3];
      if (u < F.bounds[0] || u > F.bounds[2]) break;   // :624-627
      if (v < F.bounds[1] || v > F.bounds[3]) break;
      r.proj_x = u; r.proj_y = v;                   // :629-630
      const float max_raw = F.max_dist[j];
      const float max_d = 1.2f * max_raw, min_d = 0.8f * F.min_dist[j];   // Get{Max,Min}DistanceInvariance
      const float o0 = p0 - F.Ow[0], o1 = p1 - F.Ow[1], o2 = p2 - F.Ow[2];
      const float dist = fr_norm(o0, o1, o2);
      if (dist < min_d || dist > max_d) break;      // :638
      const float view_cos = __fdiv_rn(fr_dot(o0, o1, o2, F.normal[3 * j], F.normal[3 * j + 1], F.normal[3 * j + 2]), dist);
      if (view_cos < F.cos_limit) break;            // :646
      // PredictScale: int nScale = ceil(log(ratio) / mfLogScaleFactor), clamped to the pyramid
      const float ratio = __fdiv_rn(max_raw, dist);
      int level = 0;
      if (ratio > 0.f && ratio <= 3.402823466e+38f) {
        const float c = ceilf(__fdiv_rn(logf_glibc(ratio), F.log_scale));
        if (!(c >= 0.f)) level = 0;
        else if (c >= (float)F.n_levels) level = F.n_levels - 1;
        else level = (int)c;
      }
      in_view = 1;
      r.proj_xr = u - F.mbf * invz; r.depth = pc_dist; r.view_cos = view_cos; r.level = level;   // :653-661
    } while (false);
  }
  F.in_view[i] = in_view;
  if (F.rec) F.rec[i] = r;
  if (F.valid1) {
    F.valid1[i] = in_view && !(F.far_points && r.depth > F.th_far);   // ORBmatcher.cc:52-59
    F.proj1[3 * i] = r.proj_x; F.proj1[3 * i + 1] = r.proj_y; F.proj1[3 * i + 2] = r.proj_xr;
    F.level1[i] = r.level;
    F.viewcos1[i] = r.view_cos;
  }
}

// rgbl_map_points_update: entry k of the packed arrays goes to slot[k]; slot < 0 = an entry a later one of the same slot overrides
struct PoolScatter {
  int n;
  const int32_t* slot;
  const float *wpos, *normal, *min_dist, *max_dist;   // packed, nullable
  const uint8_t* desc;
  float *p_wpos, *p_normal, *p_min, *p_max;
  uint8_t* p_desc;
};
__global__ __launch_bounds__(256) void k_map_points_scatter(PoolScatter S) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= S.n) return;
  const int j = S.slot[k];
  if (j < 0) return;
  if (S.wpos) { S.p_wpos[3 * j] = S.wpos[3 * k]; S.p_wpos[3 * j + 1] = S.wpos[3 * k + 1]; S.p_wpos[3 * j + 2] = S.wpos[3 * k + 2]; }
  if (S.normal) { S.p_normal[3 * j] = S.normal[3 * k]; S.p_normal[3 * j + 1] = S.normal[3 * k + 1]; S.p_normal[3 * j + 2] = S.normal[3 * k + 2]; }
  if (S.min_dist) S.p_min[j] = S.min_dist[k];
  if (S.max_dist) S.p_max[j] = S.max_dist[k];
  if (S.desc) {
    const uint4* src = reinterpret_cast<const uint4*>(S.desc + (size_t)k * 32);
    uint4* dst = reinterpret_cast<uint4*>(S.p_desc + (size_t)j * 32);
    const uint4 a = src[0], b = src[1];
    dst[0] = a; dst[1] = b;
  }
}

// ------------------------------------------------------------------------------------------------
// rgbl_map_points_refresh: MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:426-494) and
// MapPoint::ComputeDistinctiveDescriptors (:329-403) for pool slots whose observations are (key frame, feature) pairs of key
// frames resident on the device.  One wave per point in both kernels; grid = points, block = 64.
constexpr int kRefreshLdsRows = 128;   // a point's descriptor rows in LDS: 4 KiB per wave; longer lists take the call's scratch
struct RefreshDev {
  const int32_t *slot, *off, *obs_kf, *obs_feat;   // point p: slot[p], observations [off[p], off[p + 1])
  const int32_t *ref_kf, *ref_level;
  const float *kf_center, *scale;
  const uint8_t* kf_bad;
  const uint8_t* const* kf_desc;     // the key frames' descriptor arrays
  const int32_t* long_off;           // first row in `rows` of a point with more than kRefreshLdsRows rows, else -1
  unsigned long long* rows;
  float top_scale;                   // mvScaleFactors[nLevels - 1]
  int compute;                       // 0: the slots' present values go to the result arrays, nothing is written to the pool
  float *p_wpos, *p_normal, *p_min, *p_max;
  uint8_t* p_desc;
  float *o_normal, *o_min, *o_max;   // results, each nullable
  int32_t* o_best;
  uint8_t *o_desc, *o_wrote;
};

// The unit vectors of 64 observations at a time, one per lane, go through LDS; every lane then adds them up in list order
// (the same LDS address in all lanes: a broadcast read) - the sum is sequential as in the reference's loop, never a tree.
__global__ __launch_bounds__(64) void k_map_refresh_normal(RefreshDev R) {
  __shared__ float unit[64 * 3];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int j = R.slot[p];
  const int b = R.off[p], n = R.off[p + 1] - b;
  const bool compute = R.compute && n > 0;   // :441 a point without observations stays as it is
  const float p0 = R.p_wpos[3 * (size_t)j], p1 = R.p_wpos[3 * (size_t)j + 1], p2 = R.p_wpos[3 * (size_t)j + 2];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;        // :445 normal.setZero()
  if (compute) {
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int o = c0 + lane;
      if (o < n) {                           // :455-457 normali = Pos - Owi; normali / normali.norm()
        const float* C = R.kf_center + 3 * (size_t)R.obs_kf[b + o];
        const float d0 = p0 - C[0], d1 = p1 - C[1], d2 = p2 - C[2];
        const float len = fr_norm(d0, d1, d2);
        unit[3 * lane] = fr_quot(d0, len); unit[3 * lane + 1] = fr_quot(d1, len); unit[3 * lane + 2] = fr_quot(d2, len);
      }
      __syncthreads();
      const int m = imin(64, n - c0);
      for (int k = 0; k < m; ++k) { a0 = a0 + unit[3 * k]; a1 = a1 + unit[3 * k + 1]; a2 = a2 + unit[3 * k + 2]; }
      __syncthreads();
    }
  }
  if (lane != 0) return;
  float n0, n1, n2, dmin, dmax;
  if (compute) {
    const float* C = R.kf_center + 3 * (size_t)R.ref_kf[p];
    const float dist = fr_norm(p0 - C[0], p1 - C[1], p2 - C[2]);   // :468-469
    dmax = dist * R.scale[R.ref_level[p]];                          // :490
    dmin = fr_quot(dmax, R.top_scale);                              // :491
    const float fn = (float)n;                                      // :492 normal / n
    n0 = fr_quot(a0, fn); n1 = fr_quot(a1, fn); n2 = fr_quot(a2, fn);
    R.p_normal[3 * (size_t)j] = n0; R.p_normal[3 * (size_t)j + 1] = n1; R.p_normal[3 * (size_t)j + 2] = n2;
    R.p_min[j] = dmin; R.p_max[j] = dmax;
  } else {
    n0 = R.p_normal[3 * (size_t)j]; n1 = R.p_normal[3 * (size_t)j + 1]; n2 = R.p_normal[3 * (size_t)j + 2];
    dmin = R.p_min[j]; dmax = R.p_max[j];
  }
  if (R.o_normal) { R.o_normal[3 * (size_t)p] = n0; R.o_normal[3 * (size_t)p + 1] = n1; R.o_normal[3 * (size_t)p + 2] = n2; }
  if (R.o_min) R.o_min[p] = dmin;
  if (R.o_max) R.o_max[p] = dmax;
  if (R.o_wrote) R.o_wrote[p] = compute ? 1 : 0;
}

// observation c0 + lane of the point's list: does it contribute a descriptor row (its key frame is not bad, :352), and which
__device__ __forceinline__ bool refresh_row(const RefreshDev& R, int b, int n, int o, int* kf) {
  if (o >= n) return false;
  *kf = R.obs_kf[b + o];
  return R.kf_bad[*kf] == 0;
}

// k_distinctive's rule on `rows` gathered rows at D (LDS or the call's scratch; a row per lane, the other row of a pair
// wave-uniform: a broadcast read): median = sorted row[(N - 1) >> 1], own zero included, strict '<', the first row wins.  The
// winner goes to slot j and to the results, with its position in the point's full observation list.
__device__ __forceinline__ void refresh_pick(const RefreshDev& R, const unsigned long long* D, int rows, int p, int j, int b, int n, int lane) {
  const int k = (rows - 1) >> 1;
  uint32_t wbest = 0xffffffffu;  // median << 16 | row
  for (int r0 = 0; r0 < rows; r0 += 64) {
    const int i = r0 + lane;
    const bool live = i < rows;
    const unsigned long long* Q = D + 4 * (size_t)(live ? i : 0);
    const unsigned long long q[4] = {Q[0], Q[1], Q[2], Q[3]};
    int lo = 0, hi = 256;
    for (int it = 0; it < 9; ++it) {  // 257 possible values
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int r = 0; r < rows; ++r) c += hamming256(q, D + 4 * (size_t)r) <= mid ? 1 : 0;
      if (c >= k + 1) hi = mid; else lo = mid + 1;
    }
    const uint32_t key = wave_min_uniform(live ? ((uint32_t)lo << 16) | (uint32_t)i : 0xffffffffu);
    wbest = key < wbest ? key : wbest;
  }
  const int win = (int)(wbest & 0xffffu);
  if (lane < 4) {
    const unsigned long long v = D[4 * (size_t)win + lane];
    reinterpret_cast<unsigned long long*>(R.p_desc + (size_t)j * 32)[lane] = v;
    if (R.o_desc) reinterpret_cast<unsigned long long*>(R.o_desc + (size_t)p * 32)[lane] = v;
  }
  if (!R.o_best) return;
  for (int c0 = 0, seen = 0; c0 < n; c0 += 64) {   // the observation that gave row `win`
    int kf = 0;
    const bool good = refresh_row(R, b, n, c0 + lane, &kf);
    const unsigned long long mask = __ballot(good);
    if (good && seen + __popcll(mask & lanemask_lt()) == win) R.o_best[p] = c0 + lane;
    seen += __popcll(mask);
  }
}

__global__ __launch_bounds__(64) void k_map_refresh_desc(RefreshDev R) {
  __shared__ __attribute__((aligned(16))) unsigned long long lds_rows[kRefreshLdsRows * 4];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int j = R.slot[p];
  const int b = R.off[p], n = R.off[p + 1] - b;
  int rows = 0;
  if (R.compute && n > 0) {
    const int first = R.long_off[p];
    unsigned long long* G = first >= 0 ? R.rows + 4 * (size_t)first : nullptr;
    for (int c0 = 0; c0 < n; c0 += 64) {   // gather: the rows of the key frames that are not bad, in list order
      int kf = 0;
      const bool good = refresh_row(R, b, n, c0 + lane, &kf);
      const unsigned long long mask = __ballot(good);
      const int at = rows + __popcll(mask & lanemask_lt());
      if (good && (G || at < kRefreshLdsRows)) {
        const uint4* src = reinterpret_cast<const uint4*>(R.kf_desc[kf] + (size_t)R.obs_feat[b + c0 + lane] * 32);
        const uint4 x = src[0], y = src[1];
        if (G) { uint4* dst = reinterpret_cast<uint4*>(G + 4 * (size_t)at); dst[0] = x; dst[1] = y; }
        else { uint4* dst = reinterpret_cast<uint4*>(lds_rows + 4 * at); dst[0] = x; dst[1] = y; }
      }
      rows += __popcll(mask);
    }
    __syncthreads();
    if (rows > 0) {                        // :365 no row: the descriptor stays
      if (G) refresh_pick(R, G, rows, p, j, b, n, lane);
      else refresh_pick(R, lds_rows, rows, p, j, b, n, lane);
    }
  }
  if (rows == 0) {
    if (lane < 4 && R.o_desc) reinterpret_cast<unsigned long long*>(R.o_desc + (size_t)p * 32)[lane] = reinterpret_cast<const unsigned long long*>(R.p_desc + (size_t)j * 32)[lane];
    if (lane == 0 && R.o_best) R.o_best[p] = -1;
  }
  if (lane == 0 && R.o_wrote) R.o_wrote[p] = rows > 0 ? 1 : 0;
}

__global__ void k_test_logf(const float* x, float* y, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = logf_glibc(x[i]);
}

// ------------------------------------------------------------------------------------------------
// ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
// (/root/reference/src/ORBmatcher.cc:648-763; Tracking::MonocularInitialization, Tracking.cc:2526) with
// Frame::GetFeaturesInArea(x, y, windowSize, 0, 0) (src/Frame.cc:747-813).  The loop is sequential through
// vMatchedDistance: a level-0 feature of F1 skips every F2 candidate that an earlier feature already holds at a distance
// <= its own, and takes a candidate over from its holder otherwise.  vMatchedDistance only ever decreases, and only the
// candidates below `max_dist + 1` = the smallest d > TH_LOW with (float)d * mfNNratio > TH_LOW can change a decision (a larger
// second-best passes the ratio test like INT_MAX does, a larger best fails TH_LOW), so: the candidates of that range are
// kept in traversal order (ProjDev: proj1 = vbPrevMatched (2 floats), mpdesc1 = F1 descriptors, oct1 = F1 octaves,
// taken_by = vMatchedDistance, owner = vnMatches21), and a feature is final once no unresolved lower-index feature shares
// one of its still-available candidates - two features that share one resolve in index order, exactly the order of the loop.
template <class F>
__device__ __forceinline__ void init_available(const ProjDev& P, const int32_t* taken_by, const ListView& L, int i, F&& f) {  // f(dist, c) in traversal order
  const uint32_t r = L.cref[i];
  if (!(r & kRefOverflow)) {
    const uint32_t* e = L.clist + ref_start(r);
    for (int k = 0, n = ref_n(r); k < n; ++k) {
      const int c = entry_feature(e[k]), dist = entry_dist(e[k]);
      if (taken_by[c] > dist) f(dist, c);  // vMatchedDistance[i2] <= dist: continue (:689-690)
    }
    return;
  }
  const Desc256 d = load_desc(P.mpdesc1, i);
  for_candidates(P, P.win[i], P.rng[i], [&](int c, int) {
    const int dist = desc_dist(d, P.desc2, c);
    if (dist <= P.max_dist && taken_by[c] > dist) f(dist, c);
  });
}

// grid = ceil(n1 / 4), block = 256 = one wave per F1 feature (the candidate kernels' frame).  No blockers (the state carries no
// kStateObs), and no init_taken_by: F2 is never a resident frame here, so k_proj_grid has filled taken_by (= vMatchedDistance).
__global__ __launch_bounds__(256) void k_init_candidates(ProjDev P) {
  __shared__ unsigned long long s_keys[kPointsPerBlock][kProjCand];
  const int i = wave_point();
  if (i >= P.n1) return;
  CandResult res;
  const float x = P.proj1[2 * i], y = P.proj1[2 * i + 1];
  int4 rg = make_int4(0, 0, 0, 0);  // minLevel = maxLevel = level1 = 0
  if (P.oct1[i] == 0 && x == x && y == y && cell_window(P.grid, x, y, P.th, &rg.x, &rg.y)) {  // level1 > 0: continue (:664-666)
    const float4 w = make_float4(x, y, P.th, 0.f);
    const Desc256 d = load_desc(P.mpdesc1, i);
    res = collect_candidates(P, i, w, rg, s_keys[wave_id()], false, [&](int c, int) {
      const int dist = desc_dist(d, P.desc2, c);
      return dist <= P.max_dist ? (((unsigned long long)dist << 32) | (unsigned)c) : ~0ull;
    }, [](unsigned long long key) { return cand_entry((int)(key >> 32), 0, (int)(key & 0xffffu)); });
  }
  store_candidates(P, i, res, false);
}

// grid = 1, block = kResolveBS; state, lists, round stamps and the merged decide + commit pass as for k_proj_resolve (taken_by holds
// vMatchedDistance here).  Merging is safe for the same reason: two features that are final in one round share no available
// candidate (the higher one would have found the lower one's announcement), and lowering vMatchedDistance[c] can only take c away
// from features that were going to lose it to this one anyway - they wait behind its announcement.
template <bool LDS>
__global__ __launch_bounds__(kResolveBS) void k_init_resolve(ProjDev P) {
  __shared__ ResolveShared<LDS> sh;
  for (int c = threadIdx.x; c < P.n2; c += kResolveBS) P.owner[c] = -1;
  resolve_run<LDS>(P, sh,
    [&](const ResolveView& R, int i, int stamp) {
      if (R.state[i] != 0) return;
      const int me = (stamp << 20) | i;
      init_available(P, R.taken_by, R.L, i, [&](int, int c) { atomicMin(&R.min_unres[c], me); });
    },
    [&](const ResolveView& R, int i, int stamp) {
      if (R.state[i] != 0) return false;
      int best = INT_MAX, best2 = INT_MAX, best_idx = -1;
      bool settled = true;
      init_available(P, R.taken_by, R.L, i, [&](int dist, int c) {
        if (dist < best) { best2 = best; best = dist; best_idx = c; }  // :692-701
        else if (dist < best2) best2 = dist;
        if (lower_unresolved(R.min_unres[c], stamp, i)) settled = false;
      });
      if (!settled) return true;
      const bool ok = best <= 50 /* TH_LOW */ && (float)best < (float)best2 * P.nnratio;  // :704-706
      R.state[i] = 1;
      P.choice[i] = ok ? best_idx : -1;
      if (ok) { R.taken_by[best_idx] = best; P.owner[best_idx] = i; }  // vMatchedDistance, vnMatches21 (:713-715)
      return false;
    });
}

// ------------------------------------------------------------------------------------------------
// DBoW2 vocabulary descent: TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
// (/root/reference/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1208-1255) with FORB::distance (FORB.cpp:79-98), the
// per-feature part of Frame::ComputeBoW (src/Frame.cc:828-835).  Work-item per feature: L levels, at each level the
// child with the smallest Hamming distance (strict '<', first child wins ties).  The tree is resident on the device:
// children CSR in file order, 32-byte node descriptors.
struct VocDev {
  int n_nodes, L;
  const int32_t* child_off;
  const int32_t* child;
  const uint8_t* desc;
  const double* weight;
  const int32_t* word_id;
};
// grid = (ceil(cap / 256), frames), block = 256; d_n == nullptr: every frame holds `cap` features
__global__ __launch_bounds__(256) void k_bow_descend(VocDev V, const uint8_t* __restrict__ desc, const int32_t* __restrict__ d_n,
                                                     int cap, int levelsup, int32_t* __restrict__ word, double* __restrict__ weight,
                                                     int32_t* __restrict__ node) {
  const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  const int n = d_n ? d_n[f] : cap;
  if (i >= n || i >= cap) return;
  const size_t o = (size_t)f * cap + i;
  const unsigned long long* D = reinterpret_cast<const unsigned long long*>(desc + o * 32);
  const unsigned long long d[4] = {D[0], D[1], D[2], D[3]};
  const int nid_level = V.L - levelsup;
  int nid = 0, final_id = 0, current_level = 0;
  int b = V.child_off[0], e = V.child_off[1];
  while (b != e) {  // an inner node
    ++current_level;
    int best_d = 257;
    for (int k = b; k < e; ++k) {
      const int id = V.child[k];
      const int dist = hamming256(d, reinterpret_cast<const unsigned long long*>(V.desc + (size_t)id * 32));
      if (dist < best_d) { best_d = dist; final_id = id; }
    }
    if (current_level == nid_level) nid = final_id;
    b = V.child_off[final_id];
    e = V.child_off[final_id + 1];
  }
  word[o] = V.word_id[final_id];
  weight[o] = V.weight[final_id];
  node[o] = nid;
}

// ------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (ORBmatcher.cc:223-425), the matcher of
// Tracking::TrackReferenceKeyFrame, and the key-frame / key-frame overload (:765-905).  The vocabulary nodes shared by both
// FeatureVectors are independent problems (a feature lives in exactly one node), inside a node the key-frame features are visited in
// bucket order and a frame feature that got a match is skipped by all later ones (:296-299).  One wave per shared node: the
// key-frame features one after the other, the frame bucket spread over the lanes; best / second-best with the
// reference's order rules = minimum of (distance << 16 | bucket position) and the second order statistic.
// Two-camera frames (F.Nleft != -1, :298-326, 357-386; kRig): a key-frame feature keeps a best / second best among the node's
// LEFT frame features and a best among its RIGHT ones; the left one is taken under the usual tests, the right one - only if the
// left best passed `<= TH_LOW` - whenever its own distance does (`|| true`: no ratio test).  Both are gone for the later ones.
struct BowDev {
  const uint8_t* desc1; const uint8_t* desc2;
  const uint8_t* valid1;
  const uint8_t* valid2;  // candidates must hold a good map point as well (the key-frame / key-frame overload), or nullptr
  NodePairsDev fv;
  float nnratio;
  int max_best;           // largest accepted best distance: TH_LOW ("<=", :315) or TH_LOW - 1 ("<", :854)
  int n_left2;            // F.Nleft of a two-camera frame (k_search_by_bow_rig): features from n_left2 on belong to the right camera
  int32_t* match1;  // per key-frame feature: the frame feature it took, or -1
  int32_t* match2;  // per frame feature: the key-frame feature, or -1
};
constexpr int kBowBucket = 16384;  // frame features of one node tracked in LDS (one byte each)
struct BowShared {
  uint8_t taken[kBowBucket];  // frame features at bucket positions beyond the register trips: taken or masked out
  Desc256 q[64];              // the key-frame features' descriptors, 64 at a time, and their indices (-1: holds no map point)
  int idx1[64];
};

// The node's work for a frame bucket of up to 64 * kRegTrips features (kRegTrips = 4: any size, positions from 256 on are read from
// memory): instantiated per trip count so that a node pays for the lanes' registers it uses - the serial chain of the LARGEST node
// is the kernel's time, and with one body for all sizes every step computed four trips' distances.  The node's key-frame features
// are taken one after the other, so what sits inside that serial loop decides the kernel's time: their descriptors are staged in
// LDS 64 at a time, and instead of three dependent global loads per key-frame feature (100 -> ~15 us for a frame pair) the loop
// body is LDS reads and register work.
template <int kRegTrips, bool kRig>
__device__ __forceinline__ void bow_node(const BowDev& T, BowShared& sh, int lane, const NodeSpan& S) {
  const int b1 = S.b1, e1 = S.b1 + S.n1, b2 = S.b2, n2 = S.n2;
  const int32_t *feat1 = T.fv.feat1, *feat2 = T.fv.feat2;
  auto is_right = [&](int idx2) {
    if constexpr (kRig) return idx2 >= T.n_left2; else return false;
  };
  // the frame features at bucket positions lane, lane + 64, lane + 128, lane + 192 live in the lane's registers (index,
  // descriptor and whether the feature is taken): buckets of up to 256 features - a KITTI frame's largest hold ~100 - cost
  // neither a global nor an LDS access inside the serial loop
  for (int j = lane + 64 * kRegTrips; j < n2; j += 64) sh.taken[j] = (T.valid2 && !T.valid2[feat2[b2 + j]]) ? 1 : 0;   // beyond the register trips
  Desc256 t0[kRegTrips];
  int my_idx2[kRegTrips];
  bool gone[kRegTrips], right[kRegTrips];   // gone: taken, masked out, or no such position
#pragma unroll
  for (int r = 0; r < kRegTrips; ++r) {
    my_idx2[r] = -1;
    gone[r] = true;
    right[r] = false;
    t0[r] = Desc256{{0ull, 0ull, 0ull, 0ull}};
    if (lane + 64 * r < n2) {
      my_idx2[r] = feat2[b2 + lane + 64 * r];
      gone[r] = T.valid2 && !T.valid2[my_idx2[r]];
      right[r] = is_right(my_idx2[r]);
      t0[r] = load_desc(T.desc2, my_idx2[r]);
    }
  }
  for (int p0 = b1; p0 < e1; p0 += 64) {
    wave_sync();
    {
      const int p = p0 + lane;
      int idx1 = -1;
      if (p < e1) { idx1 = feat1[p]; if (!T.valid1[idx1]) idx1 = -1; }
      sh.idx1[lane] = idx1;
      if (idx1 >= 0) sh.q[lane] = load_desc(T.desc1, idx1);
    }
    wave_sync();
    const int cnt = imin(64, e1 - p0);
    // the next key-frame feature's descriptor is fetched from LDS while the current one is worked on
    int idx1_n = sh.idx1[0];
    Desc256 qn = sh.q[0];
    for (int k = 0; k < cnt; ++k) {
      const int idx1 = idx1_n;
      const Desc256 q = qn;
      if (k + 1 < cnt) { idx1_n = sh.idx1[k + 1]; qn = sh.q[k + 1]; }
      if (idx1 < 0) continue;  // wave-uniform
      uint32_t best = 0xffffffffu;  // dist << 16 | bucket position (kRig: among the left camera's)
      uint32_t second = 256;
      uint32_t best_r = 0xffffffffu;  // kRig, right camera: the first minimum is all that is used
      // best / second-best without a branch (the loop body is what a node's serial chain is made of): the smaller key stays, the
      // larger one's distance competes for second place - the key it displaces when it is the new best (second >= best's distance
      // always), itself otherwise; an absent candidate is the key 0xffffffff and changes nothing
      auto visit = [&](uint32_t key, bool is_r) {
        if constexpr (kRig) {
          best_r = (is_r && key < best_r) ? key : best_r;
          key = is_r ? 0xffffffffu : key;
        }
        const uint32_t lo = key < best ? key : best, hi = key < best ? best : key;
        second = (hi >> 16) < second ? (hi >> 16) : second;
        best = lo;
      };
#pragma unroll
      for (int r = 0; r < kRegTrips; ++r) {
        if (64 * r >= n2) break;  // wave-uniform
        const uint32_t key = ((uint32_t)desc_dist(q, t0[r]) << 16) | (uint32_t)(lane + 64 * r);
        visit(gone[r] ? 0xffffffffu : key, right[r]);
      }
      for (int j = lane + 64 * kRegTrips; j < n2; j += 64) {
        if (sh.taken[j]) continue;
        const int idx2 = feat2[b2 + j];
        visit(((uint32_t)desc_dist(q, T.desc2, idx2) << 16) | (uint32_t)j, is_right(idx2));
      }
      // wave-wide: the smallest key, and the smallest distance among everything else
      const uint32_t wbest = wave_min_uniform(best);   // register-file DPP steps: the reductions sit in the node's serial loop
      const int other = (int)wave_min_uniform(best == wbest ? second : (best == 0xffffffffu ? 256u : best >> 16));
      uint32_t wbest_r = 0xffffffffu;
      if constexpr (kRig) wbest_r = wave_min_uniform(best_r);
      const int best_dist = (int)(wbest >> 16);
      if (wbest == 0xffffffffu || best_dist > T.max_best) continue;   // :315: the right camera's match sits inside this test
      // the lane that holds the feature's index takes it (wave-uniform call); true: the position is one of sh.taken
      auto take = [&](uint32_t wkey, bool left) {
        const int pos = (int)(wkey & 0xffffu);
        if (lane == (pos & 63)) {
          int idx2 = -1;
#pragma unroll
          for (int r = 0; r < kRegTrips; ++r)
            if ((pos >> 6) == r) { idx2 = my_idx2[r]; gone[r] = true; }
          if (pos >= 64 * kRegTrips) { idx2 = feat2[b2 + pos]; sh.taken[pos] = 1; }
          if (left) T.match1[idx1] = idx2;   // kRig: the result is match2; match1 keeps the left camera's feature
          T.match2[idx2] = idx1;
        }
        return pos >= 64 * kRegTrips;
      };
      bool beyond = false;
      if ((float)best_dist < T.nnratio * (float)other) beyond = take(wbest, true);
      if constexpr (kRig)
        if (wbest_r != 0xffffffffu && (int)(wbest_r >> 16) <= T.max_best) beyond = take(wbest_r, false) || beyond;
      if (beyond) wave_sync();   // wave-uniform
    }
  }
}

// grid = shared nodes, block = 64: a lane keeps the descriptor of ITS frame feature (bucket position = lane, every bucket of a KITTI
// frame's ~100 nodes fits one trip) in registers.  Both kernels choose the node body by the frame bucket's size.
template <bool kRig>
__device__ __forceinline__ void bow_dispatch(const BowDev& T, BowShared& sh) {
  const NodeSpan S = node_span(T.fv);
  const int lane = threadIdx.x;
  if (S.n2 <= 64) bow_node<1, kRig>(T, sh, lane, S);
  else if (S.n2 <= 128) bow_node<2, kRig>(T, sh, lane, S);
  else if (S.n2 <= 192) bow_node<3, kRig>(T, sh, lane, S);
  else bow_node<4, kRig>(T, sh, lane, S);
}
__global__ __launch_bounds__(64) void k_search_by_bow(BowDev T) {
  __shared__ BowShared sh;
  bow_dispatch<false>(T, sh);
}
__global__ __launch_bounds__(64) void k_search_by_bow_rig(BowDev T) {   // a two-camera frame
  __shared__ BowShared sh;
  bow_dispatch<true>(T, sh);
}

}  // namespace rgbl

using namespace rgbl;

namespace {
// RGBL_BF_MFMA=0 selects the VALU popcount scan (k_hamming_bf) instead of the matrix-core one, =i8 the i8 instruction
// (k_hamming_mfma) instead of the block-scaled FP4 one (k_hamming_fp4, the default): read when the handle is created.
inline bool bf_on_matrix_cores(const rgbl_matcher* m) { return m->bf_matrix; }
inline bool bf_on_fp4(const rgbl_matcher* m) { return m->bf_fp4; }
// A key frame's FeatureVector (CSR): the resident copy when its frame holds one of the same shape
// (rgbl_device_frame_set_feature_vector since the last upload / capture), else staged.
void put_feature_vector(HostCall& hc, const rgbl_keyframe_view* v, const int32_t** d_off, const int32_t** d_feat) {
  const int nf = v->node_off[v->n_nodes];
  if (v->device && v->device->n_nodes == v->n_nodes && v->device->nf == nf) {
    *d_off = v->device->d_fv; *d_feat = v->device->d_fv + v->n_nodes + 1;
    return;
  }
  hc.put(d_off, v->node_off, (size_t)v->n_nodes + 1);
  hc.put(d_feat, v->node_feat, (size_t)nf);
}

// What a search over two FeatureVectors starts from (SearchForTriangulation, SearchByBoW): the vocabulary nodes both sorted
// vectors share, in the order of the reference's merge walk (ORBmatcher.cc:243-246, 388-401; 963-968, 1103-1116).
struct FeatDst { const uint8_t** desc; const float** xy; const int32_t** oct; const float** ur; };   // null: the kernel does not read it
struct SharedNodes {
  const rgbl_keyframe_view *a, *b;
  std::vector<int32_t> pa, pb;   // positions of the shared nodes in a's and b's node lists
  SharedNodes(const rgbl_keyframe_view* a_, const rgbl_keyframe_view* b_) : a(a_), b(b_) {
    for (int i = 0, j = 0; i < a->n_nodes && j < b->n_nodes;) {
      if (a->node_id[i] == b->node_id[j]) { pa.push_back(i++); pb.push_back(j++); }
      else if (a->node_id[i] < b->node_id[j]) ++i;
      else ++j;
    }
  }
  int npairs() const { return (int)pa.size(); }
  bool empty() const { return pa.empty() || a->n == 0 || b->n == 0; }   // nothing to launch
  // inside the call's layout: both sides' per-feature arrays and FeatureVectors (resident or staged), then the pair lists
  int put(HostCall& hc, FeatDst d1, FeatDst d2, NodePairsDev& N) const {
    RGBL_TRY(put_first(hc, a, d1, N));
    return put_second(hc, d2, N);
  }
  // the two halves of put(): a chain of searches from one first key frame (rgbl_create_new_map_points) stages it once
  static int put_first(HostCall& hc, const rgbl_keyframe_view* a, FeatDst d1, NodePairsDev& N) {
    RGBL_TRY(put_features(hc, a->device, a->n, a->desc, a->kp_xy, a->kp_octave, a->uright, d1.desc, d1.xy, d1.oct, d1.ur));
    put_feature_vector(hc, a, &N.off1, &N.feat1);
    return RGBL_OK;
  }
  int put_second(HostCall& hc, FeatDst d2, NodePairsDev& N) const {
    RGBL_TRY(put_features(hc, b->device, b->n, b->desc, b->kp_xy, b->kp_octave, b->uright, d2.desc, d2.xy, d2.oct, d2.ur));
    put_feature_vector(hc, b, &N.off2, &N.feat2);
    hc.put(&N.pair_n1, pa.data(), pa.size());
    hc.put(&N.pair_n2, pb.data(), pb.size());
    return RGBL_OK;
  }
};

// The rotation-consistency check (e.g. ORBmatcher.cc:1083-1096, 1119-1136): add() bins an item by angle_a - angle_b in the
// order the caller visits it; drop_outliers() hands every item outside the bins ComputeThreeMaxima keeps (:2012-2053) to drop.
struct RotationFilter {
  std::vector<int> hist[30];
  void add(int item, float angle_a, float angle_b) {
    float rot = angle_a - angle_b;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / 30));
    if (bin == 30) bin = 0;
    if (bin >= 0 && bin < 30) hist[bin].push_back(item);
  }
  template <class Drop> void drop_outliers(Drop drop) const {
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < 30; ++i) {
      const int sz = (int)hist[i].size();
      if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; i3 = i2; i2 = i1; i1 = i; }
      else if (sz > max2) { max3 = max2; max2 = sz; i3 = i2; i2 = i; }
      else if (sz > max3) { max3 = sz; i3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if (max3 < 0.1f * (float)max1) { i3 = -1; }
    for (int i = 0; i < 30; ++i)
      if (i != i1 && i != i2 && i != i3)
        for (int item : hist[i]) drop(item);
  }
};

// What is left to do once matches12[idx1] (a's feature -> b's, or -1) is filled: count, the rotation check with its bins filled in
// the order the reference visits idx1 - node by node in merge order, bucket order (ORBmatcher.cc:1083-1096, 1119-1136; 855-865, 886-901) -
// and *out_nmatches.
// The launch of one SearchForTriangulation once T's arrays are laid out: the call's parameters, then one workgroup per shared node.
int enqueue_triangulation(rgbl_matcher* m, hipStream_t s, TriDev& T, const rgbl_triangulation_params* prm, int npairs) {
  memcpy(T.F, prm->F12, sizeof(T.F));
  T.ep[0] = prm->epipole[0];
  T.ep[1] = prm->epipole[1];
  T.only_stereo = prm->only_stereo;
  T.coarse = prm->coarse;
  RGBL_TRY(launch(m, s, "k_search_triangulation", k_search_triangulation, dim3(npairs), dim3(256), 0, T));
  return RGBL_OK;
}

void finish_matches12(const SharedNodes& sn, int32_t* matches12, bool check_orientation, int* out_nmatches) {
  int nmatches = 0;
  for (int i = 0; i < sn.a->n; ++i) nmatches += matches12[i] >= 0;
  if (check_orientation) {
    RotationFilter rf;
    for (int p = 0; p < sn.npairs(); ++p)
      for (int q = sn.a->node_off[sn.pa[p]]; q < sn.a->node_off[sn.pa[p] + 1]; ++q) {
        const int idx1 = sn.a->node_feat[q];
        if (matches12[idx1] >= 0) rf.add(idx1, sn.a->kp_angle[idx1], sn.b->kp_angle[matches12[idx1]]);
      }
    rf.drop_outliers([&](int idx1) { matches12[idx1] = -1; --nmatches; });
  }
  *out_nmatches = nmatches;
}

}  // namespace

extern "C" {

int rgbl_matcher_create(int device, rgbl_matcher** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (rgbl_device_count() <= device || device < 0) {
    set_error("no usable HIP device %d (this library has no CPU fallback)", device);
    return RGBL_ERR_NO_DEVICE;
  }
  RGBL_HIP(hipSetDevice(device));
  rgbl_matcher* m = new rgbl_matcher;
  m->device = device;
  if (const char* v = getenv("RGBL_BF_MFMA")) { m->bf_matrix = v[0] != '0'; m->bf_fp4 = v[0] != 'i'; }
  if (const char* v = getenv("RGBL_BF_SPLIT")) m->bf_split = v[0] != '0';
  if (const char* v = getenv("RGBL_GBA_PANEL")) m->gba_panel = atoi(v) == 16 ? 16 : atoi(v) == 64 ? 64 : 32;
  if (hipStreamCreate(&m->own_stream) != hipSuccess) { delete m; set_error("hipStreamCreate failed"); return RGBL_ERR_HIP; }
  m->stream = m->own_stream;
  *out = m;
  return RGBL_OK;
}

void rgbl_matcher_destroy(rgbl_matcher* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  m->timer.collect();
  if (m->d_buf) (void)hipFree(m->d_buf);
  if (m->h_pin) (void)hipHostFree(m->h_pin);
  if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
  delete m;
}

// Pool of matcher handles.  The reference builds its ORBmatcher as a function-local object in every Tracking / LocalMapping /
// LoopClosing call (Tracking.cc:2525, 2761, 2890, 3424, 3662, 3701; LocalMapping.cc:412): a drop-in class that created a HIP
// stream (and later freed a device arena, which synchronises the whole device) per object would pay that several times per
// frame.  acquire() hands out an idle handle of the device or creates one; release() parks it again - stream and arena stay
// alive for the life of the process.  Handles in use at the same time are distinct, so concurrent callers keep overlapping.
namespace {
struct MatcherPool {
  std::mutex mu;
  std::vector<rgbl_matcher*> idle;
};
MatcherPool* matcher_pool_ptr() {
  static MatcherPool* pool = new MatcherPool;  // never destroyed: no HIP calls from static destructors
  return pool;
}
}  // namespace

int rgbl_matcher_acquire(int device, rgbl_matcher** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  {
    MatcherPool& P = *matcher_pool_ptr();
    std::lock_guard<std::mutex> lock(P.mu);
    for (size_t i = 0; i < P.idle.size(); ++i)
      if (P.idle[i]->device == device) {
        *out = P.idle[i];
        P.idle.erase(P.idle.begin() + (long)i);
        return RGBL_OK;
      }
  }
  return rgbl_matcher_create(device, out);
}

void rgbl_matcher_release(rgbl_matcher* m) {
  if (!m) return;
  if (m->stream != m->own_stream) {  // a borrowed stream must not outlive its owner's wishes
    (void)hipStreamSynchronize(m->stream);
    m->stream = m->own_stream;
  }
  if (m->timer.enabled || !m->timer.recs.empty()) {  // the next owner must not inherit profiling brackets
    (void)hipStreamSynchronize(m->stream);
    m->timer.collect();
    m->timer.enabled = false;
  }
  m->timer.reset();
  MatcherPool& P = *matcher_pool_ptr();
  std::lock_guard<std::mutex> lock(P.mu);
  P.idle.push_back(m);
}

int rgbl_matcher_pool_clear(void) {
  std::vector<rgbl_matcher*> idle;
  {
    MatcherPool& P = *matcher_pool_ptr();
    std::lock_guard<std::mutex> lock(P.mu);
    idle.swap(P.idle);
  }
  for (rgbl_matcher* m : idle) rgbl_matcher_destroy(m);
  return (int)idle.size();
}

int rgbl_matcher_pool_size(void) {
  MatcherPool& P = *matcher_pool_ptr();
  std::lock_guard<std::mutex> lock(P.mu);
  return (int)P.idle.size();
}

// ---- frames resident on the device (include/rgbl_frontend.h) -----------------------------------------------------------
int rgbl_device_frame_create(int device, int capacity, rgbl_device_frame** out) {
  if (!out || capacity < 1 || capacity > 65535) { set_error("device frame: capacity 1 .. 65535"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (rgbl_device_count() <= device || device < 0) {
    set_error("no usable HIP device %d (this library has no CPU fallback)", device);
    return RGBL_ERR_NO_DEVICE;
  }
  RGBL_HIP(hipSetDevice(device));
  rgbl_device_frame* f = new rgbl_device_frame;
  f->device = device;
  f->cap = (capacity + 63) / 64 * 64;   // every array starts 256-byte aligned
  const size_t cap = (size_t)f->cap;
  if (rgbl::device_alloc(&f->block, cap * 48) != hipSuccess || hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&f->ready, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    rgbl_device_frame_destroy(f);
    set_error("device frame: allocation failed");
    return RGBL_ERR_HIP;
  }
  f->d_desc = f->block;
  f->d_xy = reinterpret_cast<float*>(f->block + cap * 32);
  f->d_oct = reinterpret_cast<int32_t*>(f->block + cap * 40);
  f->d_ur = reinterpret_cast<float*>(f->block + cap * 44);
  RGBL_HIP(hipEventRecord(f->ready, f->stream));
  *out = f;
  return RGBL_OK;
}

void rgbl_device_frame_destroy(rgbl_device_frame* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->ready) { (void)hipEventSynchronize(f->ready); (void)hipEventDestroy(f->ready); }
  if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
  if (f->block) (void)hipFree(f->block);
  if (f->d_fv) (void)hipFree(f->d_fv);
  if (f->d_cell_start) (void)hipFree(f->d_cell_start);   // the grid's block
  if (f->h_pin) (void)hipHostFree(f->h_pin);
  delete f;
}

static int frame_pin(rgbl_device_frame* f, size_t bytes) {
  if (bytes <= f->pin_size) return RGBL_OK;
  if (f->h_pin) { (void)hipHostFree(f->h_pin); f->h_pin = nullptr; f->pin_size = 0; }
  RGBL_HIP(rgbl::pinned_alloc(&f->h_pin, bytes));
  f->pin_size = bytes;
  return RGBL_OK;
}

int rgbl_device_frame_upload(rgbl_device_frame* f, int n, const uint8_t* desc, const float* kp_xy, const int32_t* kp_octave,
                             const float* uright) {
  if (!f || n < 0 || n > f->cap || (n > 0 && (!desc || !kp_xy || !kp_octave))) { set_error("device frame upload: invalid argument / more features than the capacity"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(f->device));
  const size_t cap = (size_t)f->cap;
  RGBL_TRY(frame_pin(f, cap * 48));
  (void)hipEventSynchronize(f->ready);   // nothing still fills the arrays from elsewhere
  memcpy(f->h_pin, desc, (size_t)n * 32);
  memcpy(f->h_pin + cap * 32, kp_xy, (size_t)n * 8);
  memcpy(f->h_pin + cap * 40, kp_octave, (size_t)n * 4);
  float* ur = reinterpret_cast<float*>(f->h_pin + cap * 44);
  if (uright) memcpy(ur, uright, (size_t)n * 4);
  else for (int i = 0; i < n; ++i) ur[i] = -1.f;
  // the mirror has the block's layout: one request for all four arrays
  RGBL_HIP(hipMemcpyAsync(f->block, f->h_pin, cap * 44 + (size_t)n * 4, hipMemcpyHostToDevice, f->stream));
  RGBL_HIP(hipEventRecord(f->ready, f->stream));
  RGBL_HIP(hipStreamSynchronize(f->stream));   // the mirror is reused by the next upload; the caller's arrays are free at once anyway
  f->n = n;
  f->has_grid = false; f->n_nodes = -1; f->nf = 0;   // new keypoints: rgbl_device_frame_set_grid / _set_feature_vector again
  return RGBL_OK;
}

int rgbl_device_frame_set_feature_vector(rgbl_device_frame* f, int n_nodes, const int32_t* node_off, const int32_t* node_feat) {
  if (!f || n_nodes < 0 || !node_off || node_off[0] != 0) { set_error("device frame: invalid FeatureVector"); return RGBL_ERR_INVALID; }
  const int nf = node_off[n_nodes];
  if (nf < 0 || nf > f->cap || (nf > 0 && !node_feat)) { set_error("device frame: FeatureVector with %d entries, capacity %d", nf, f->cap); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(f->device));
  const int words = n_nodes + 1 + nf;
  if (words > f->fv_cap) {
    if (f->d_fv) { RGBL_HIP(hipStreamSynchronize(f->stream)); (void)hipFree(f->d_fv); f->d_fv = nullptr; f->fv_cap = 0; }
    const int cap = std::max(words, 2 * f->cap + 2);
    RGBL_HIP(rgbl::device_alloc(&f->d_fv, sizeof(int32_t) * (size_t)cap));
    f->fv_cap = cap;
  }
  RGBL_TRY(frame_pin(f, std::max((size_t)f->cap * 48, sizeof(int32_t) * (size_t)words)));
  (void)hipEventSynchronize(f->ready);
  int32_t* h = reinterpret_cast<int32_t*>(f->h_pin);
  memcpy(h, node_off, sizeof(int32_t) * ((size_t)n_nodes + 1));
  if (nf) memcpy(h + n_nodes + 1, node_feat, sizeof(int32_t) * (size_t)nf);
  RGBL_HIP(hipMemcpyAsync(f->d_fv, h, sizeof(int32_t) * (size_t)words, hipMemcpyHostToDevice, f->stream));
  RGBL_HIP(hipEventRecord(f->ready, f->stream));
  RGBL_HIP(hipStreamSynchronize(f->stream));
  f->n_nodes = n_nodes; f->nf = nf;
  return RGBL_OK;
}

int rgbl_device_frame_set_grid(rgbl_device_frame* f, const float grid[6]) {
  if (!f || !grid) { set_error("device frame: null argument"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(f->device));
  if (!f->d_cell_start) {   // one block: cell_start [kGridCells + 1] | cell_items [cap] | scratch [cap], 256-byte aligned
    const size_t items = (sizeof(uint32_t) * (kGridCells + 1) + 255) / 256 * 256;
    const size_t scratch = items + (sizeof(uint16_t) * (size_t)f->cap + 255) / 256 * 256;
    uint8_t* block = nullptr;
    RGBL_HIP(rgbl::device_alloc(&block, scratch + sizeof(int32_t) * (size_t)f->cap));
    f->d_cell_start = reinterpret_cast<uint32_t*>(block);
    f->d_cell_items = reinterpret_cast<uint16_t*>(block + items);
    f->d_grid_scratch = reinterpret_cast<int32_t*>(block + scratch);
  }
  ProjDev P;
  memset(&P, 0, sizeof(P));
  P.n2 = f->n; P.xy2 = f->d_xy;
  memcpy(P.grid, grid, sizeof(P.grid));
  P.cell_start = f->d_cell_start; P.cell_items = f->d_cell_items; P.taken_by = f->d_grid_scratch;
  RGBL_HIP(hipStreamWaitEvent(f->stream, f->ready, 0));   // the keypoints may still be on their way (capture)
  launch_proj_grid(P, f->stream);
  RGBL_HIP(hipGetLastError());
  RGBL_HIP(hipEventRecord(f->ready, f->stream));
  RGBL_HIP(hipStreamSynchronize(f->stream));
  memcpy(f->grid, grid, sizeof(f->grid));
  f->has_grid = true;
  return RGBL_OK;
}

int rgbl_device_frame_size(const rgbl_device_frame* f) { return f ? f->n : 0; }

int rgbl_device_frame_download(rgbl_device_frame* f, uint8_t* desc, float* kp_xy, int32_t* kp_octave, float* uright) {
  if (!f) { set_error("null frame"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(f->device));
  RGBL_HIP(hipEventSynchronize(f->ready));
  const size_t n = (size_t)f->n;
  if (desc && n) RGBL_HIP(hipMemcpy(desc, f->d_desc, n * 32, hipMemcpyDeviceToHost));
  if (kp_xy && n) RGBL_HIP(hipMemcpy(kp_xy, f->d_xy, n * 8, hipMemcpyDeviceToHost));
  if (kp_octave && n) RGBL_HIP(hipMemcpy(kp_octave, f->d_oct, n * 4, hipMemcpyDeviceToHost));
  if (uright && n) RGBL_HIP(hipMemcpy(uright, f->d_ur, n * 4, hipMemcpyDeviceToHost));
  return RGBL_OK;
}

int rgbl_matcher_sync(rgbl_matcher* m) {
  if (!m) { set_error("null handle"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(m->device));
  RGBL_HIP(hipStreamSynchronize(m->stream));
  m->timer.collect();
  return RGBL_OK;
}
int rgbl_matcher_set_stream(rgbl_matcher* m, void* hip_stream) {
  if (!m) { set_error("null handle"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipStreamSynchronize(m->stream));
  m->stream = hip_stream ? (hipStream_t)hip_stream : m->own_stream;
  return RGBL_OK;
}
void* rgbl_matcher_stream(rgbl_matcher* m) { return m ? (void*)m->stream : nullptr; }
int rgbl_matcher_profile(rgbl_matcher* m, int enable) {
  if (!m) { set_error("null handle"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipStreamSynchronize(m->stream));
  m->timer.reset();
  m->timer.enabled = enable != 0;
  return RGBL_OK;
}
int rgbl_matcher_profile_read(rgbl_matcher* m, const char** names, double* total_ms, long* launches, int cap) {
  if (!m) return 0;
  (void)hipStreamSynchronize(m->stream);
  m->timer.collect();
  const int n = (int)m->timer.names.size();
  for (int i = 0; i < n && i < cap; ++i) {
    if (names) names[i] = m->timer.names[i].c_str();
    if (total_ms) total_ms[i] = m->timer.total_ms[i];
    if (launches) launches[i] = m->timer.count[i];
  }
  return n;
}
int rgbl_matcher_profile_samples(rgbl_matcher* m, int kernel, float* ms, int cap) {
  if (!m || (cap > 0 && !ms)) return 0;
  (void)hipStreamSynchronize(m->stream);
  m->timer.collect();
  return m->timer.read_samples(kernel, ms, cap);
}

int rgbl_descriptor_distance(const uint8_t* a, const uint8_t* b) {
  // host helper with the reference's word-wise semantics (8 x 32-bit little-endian words)
  int dist = 0;
  for (int i = 0; i < 8; ++i) {
    uint32_t wa, wb;
    memcpy(&wa, a + 4 * i, 4);
    memcpy(&wb, b + 4 * i, 4);
    dist += __builtin_popcount(wa ^ wb);
  }
  return dist;
}

int rgbl_hamming_bf_batch_device(rgbl_matcher* m, const uint8_t* d_desc, const int32_t* d_n, int cap, const int32_t* d_pair_a,
                                 const int32_t* d_pair_b, int n_pairs, int32_t* d_best_idx, int32_t* d_best_dist,
                                 int32_t* d_second_dist) {
  if (!m || !d_desc || !d_n || !d_pair_a || !d_pair_b || !d_best_idx || !d_best_dist || cap < 1 || cap > 65535 || n_pairs < 0) {
    set_error("invalid argument (cap 1 .. 65535: a train row's index travels in 16 bits)");
    return RGBL_ERR_INVALID;
  }
  if (n_pairs == 0) return RGBL_OK;
  RGBL_HIP(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const dim3 grid = xcd_grid(true, (cap + kBfQueriesPerBlock - 1) / kBfQueriesPerBlock, n_pairs);
  if (!bf_on_matrix_cores(m))
    return launch(m, s, "k_hamming_bf", k_hamming_bf, dim3((cap + 63) / 64, n_pairs), dim3(256), 0, d_desc, d_n, cap, d_pair_a, d_pair_b, d_best_idx, d_best_dist, d_second_dist);
  if (!bf_on_fp4(m))
    return launch(m, s, "k_hamming_mfma", k_hamming_mfma, grid, dim3(256), 0, d_desc, d_n, cap, d_pair_a, d_pair_b, d_best_idx, d_best_dist, d_second_dist);
  return launch(m, s, "k_hamming_fp4", k_hamming_fp4, grid, dim3(256), 0, d_desc, d_n, cap, d_pair_a, d_pair_b, d_best_idx, d_best_dist, d_second_dist, 1, (uint32_t*)nullptr);
}

int rgbl_hamming_bf(rgbl_matcher* m, const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb, int32_t* best_idx,
                    int32_t* best_dist, int32_t* second_dist) {
  if (!m || na < 0 || nb < 0 || nb > 65535 || (na > 0 && (!desc_a || !best_idx || !best_dist)) || (nb > 0 && !desc_b)) {
    set_error("invalid argument (at most 65535 train descriptors: a train row's index travels in 16 bits)");
    return RGBL_ERR_INVALID;
  }
  if (na == 0) return RGBL_OK;
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  const int cap = std::max(std::max(na, nb), 1);
  // One pair per call: the query blocks alone (8 for 2000 descriptors) would leave most of the chip idle, so the train set is
  // cut into slices of whole stages, one launch slice each, folded by k_hamming_merge (FP4 kernel only).
  const int qblocks = (na + kBfQueriesPerBlock - 1) / kBfQueriesPerBlock, stages = (nb + kBfStageRowsF4 - 1) / kBfStageRowsF4;
  int splits = 1;
  if (bf_on_matrix_cores(m) && bf_on_fp4(m) && m->bf_split)
    splits = std::max(1, std::min(std::min(16, stages / 4), 128 / std::max(qblocks, 1)));
  HostCall hc(m);
  hipStream_t s = hc.s;
  const int32_t counts[2] = {na, nb};
  const uint8_t* d_desc = nullptr;
  const int32_t* d_n = nullptr;
  int32_t *d_bi = nullptr, *d_bd = nullptr, *d_sd = nullptr;
  uint32_t* d_partial = nullptr;
  RGBL_TRY(hc.begin([&]() -> int {
    // both descriptor sets and the counts in one block, ONE request up; the three result arrays come back with one
    d_desc = hc.stage<uint8_t>((size_t)2 * cap * 32, [&](uint8_t* h) {
      memcpy(h, desc_a, (size_t)na * 32);
      if (nb > 0) memcpy(h + (size_t)cap * 32, desc_b, (size_t)nb * 32);
    });
    hc.put(&d_n, counts, 2);
    d_bi = hc.result<int32_t>(na);
    d_bd = hc.result<int32_t>(na);
    d_sd = hc.result<int32_t>(na);
    d_partial = hc.scratch<uint32_t>((size_t)splits * na * 2);
    return RGBL_OK;
  }));
  // pair_a/pair_b == NULL selects the fixed pair (frame 0 -> frame 1)
  if (bf_on_matrix_cores(m)) {
    m->timer.begin(bf_on_fp4(m) ? "k_hamming_fp4" : "k_hamming_mfma", s);
    if (bf_on_fp4(m)) {
      hipLaunchKernelGGL(k_hamming_fp4, xcd_grid(false, qblocks, splits), dim3(256), 0, s, d_desc, d_n, cap, (const int32_t*)nullptr,
                         (const int32_t*)nullptr, d_bi, d_bd, d_sd, splits, d_partial);
      if (splits > 1) hipLaunchKernelGGL(k_hamming_merge, dim3((na + 255) / 256), dim3(256), 0, s, d_partial, na, splits, d_bi, d_bd, d_sd);
    } else {
      hipLaunchKernelGGL(k_hamming_mfma, xcd_grid(false, qblocks, 1), dim3(256), 0, s, d_desc, d_n, cap, (const int32_t*)nullptr,
                         (const int32_t*)nullptr, d_bi, d_bd, d_sd);
    }
  } else {
    m->timer.begin("k_hamming_bf", s);
    hipLaunchKernelGGL(k_hamming_bf, dim3((na + 63) / 64, 1), dim3(256), 0, s, d_desc, d_n, cap, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, d_bi, d_bd, d_sd);
  }
  m->timer.end(s);
  RGBL_HIP(hipGetLastError());
  RGBL_TRY(hc.fetch());
  memcpy(best_idx, hc.host(d_bi), sizeof(int32_t) * na);
  memcpy(best_dist, hc.host(d_bd), sizeof(int32_t) * na);
  if (second_dist) memcpy(second_dist, hc.host(d_sd), sizeof(int32_t) * na);
  return RGBL_OK;
}

int rgbl_stereo_fisheye_matches(rgbl_matcher* m, const uint8_t* desc_left, int n_left, int mono_left, const uint8_t* desc_right,
                                int n_right, int mono_right, int32_t* left_to_right, int32_t* best_dist, int32_t* second_dist) {
  // Frame::ComputeStereoFishEyeMatches (/root/reference/src/Frame.cc:1256-1296) up to the triangulation: the lapping-area
  // subsets [mono, n) of both descriptor sets, cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) = best and second-best train
  // row of every query (strict '<': the lower index stays in front on ties), then Lowe's ratio
  // `matches.size() >= 2 && best < second * 0.7` (float times double, compared in double)
  if (!m || n_left < 0 || n_right < 0 || mono_left < 0 || mono_right < 0 || mono_left > n_left || mono_right > n_right ||
      (n_left > 0 && (!desc_left || !left_to_right)) || (n_right > 0 && !desc_right)) {
    set_error("invalid argument");
    return RGBL_ERR_INVALID;
  }
  for (int i = 0; i < n_left; ++i) {
    left_to_right[i] = -1;
    if (best_dist) best_dist[i] = 256;
    if (second_dist) second_dist[i] = 256;
  }
  const int nq = n_left - mono_left, nt = n_right - mono_right;
  if (nq == 0 || nt == 0) return RGBL_OK;
  std::vector<int32_t> bi(nq), bd(nq), sd(nq);
  RGBL_TRY(rgbl_hamming_bf(m, desc_left + (size_t)mono_left * 32, nq, desc_right + (size_t)mono_right * 32, nt, bi.data(), bd.data(),
                           sd.data()));
  for (int i = 0; i < nq; ++i) {
    if (best_dist) best_dist[mono_left + i] = bd[i];
    if (second_dist) second_dist[mono_left + i] = nt >= 2 ? sd[i] : 256;
    if (nt >= 2 && (double)(float)bd[i] < (double)(float)sd[i] * 0.7) left_to_right[mono_left + i] = bi[i] + mono_right;
  }
  return RGBL_OK;
}

void rgbl_fundamental(const float K1[4], const float K2[4], const float R12[9], const float t12[3], float F12[9]) {
  // Pinhole.cpp:109-112: K1^T^-1 * hat(t12) * R12 * K2^-1 in fp32; Eigen evaluates 3x3 products coefficient-wise
  // as p0 + (p1 + p2) and inverts 3x3 matrices through cofactors (determinant from column 0).
  auto mul = [](const float* A, const float* B, float* C) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const float p0 = A[3 * r] * B[c], p1 = A[3 * r + 1] * B[3 + c], p2 = A[3 * r + 2] * B[6 + c];
        C[3 * r + c] = p0 + (p1 + p2);
      }
  };
  auto cof = [](const float* m, int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1];
  };
  auto inv = [&](const float* m, float* r) {
    const float c0 = cof(m, 0, 0), c1 = cof(m, 1, 0), c2 = cof(m, 2, 0);
    const float det = c0 * m[0] + (c1 * m[3] + c2 * m[6]);
    const float id = 1.0f / det;
    r[0] = c0 * id; r[1] = c1 * id; r[2] = c2 * id;
    r[3] = cof(m, 0, 1) * id; r[4] = cof(m, 1, 1) * id; r[5] = cof(m, 2, 1) * id;
    r[6] = cof(m, 0, 2) * id; r[7] = cof(m, 1, 2) * id; r[8] = cof(m, 2, 2) * id;
  };
  const float k1t[9] = {K1[0], 0.f, 0.f, 0.f, K1[1], 0.f, K1[2], K1[3], 1.f};
  const float k2[9] = {K2[0], 0.f, K2[2], 0.f, K2[1], K2[3], 0.f, 0.f, 1.f};
  const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
  float a[9], b[9], c[9], k2i[9];
  inv(k1t, a);
  mul(a, tx, b);
  mul(b, R12, c);
  inv(k2, k2i);
  mul(c, k2i, F12);
}

int rgbl_search_triangulation(rgbl_matcher* m, const rgbl_keyframe_view* k1, const rgbl_keyframe_view* k2,
                              const rgbl_triangulation_params* prm, int32_t* matches12, int* out_nmatches) {
  if (!m || !k1 || !k2 || !prm || !matches12 || !out_nmatches || k1->n < 0 || k2->n < 0 || prm->n_levels < 1) {
    set_error("invalid argument");
    return RGBL_ERR_INVALID;
  }
  *out_nmatches = 0;
  const int n1 = k1->n, n2 = k2->n;
  for (int i = 0; i < n1; ++i) matches12[i] = -1;
  const SharedNodes sn(k1, k2);
  if (!sn.empty()) {
    RGBL_HIP(hipSetDevice(m->device));
    StreamDrain drain(m->stream);  // error returns included
    HostCall hc(m);
    hipStream_t s = hc.s;
    TriDev T;
    RGBL_TRY(hc.begin([&]() -> int {
      RGBL_TRY(sn.put(hc, {&T.desc1, &T.xy1, nullptr, &T.ur1}, {&T.desc2, &T.xy2, &T.oct2, &T.ur2}, T.fv));
      hc.put(&T.mp1, k1->has_mappoint, (size_t)n1);
      hc.put(&T.mp2, k2->has_mappoint, (size_t)n2);
      hc.put(&T.scale2, prm->scale_factors2, (size_t)prm->n_levels);
      hc.put(&T.sigma2, prm->level_sigma2_2, (size_t)prm->n_levels);
      T.matches12 = hc.put_fill<int32_t>(n1, 0xff);   // all -1: travels with the upload
      hc.mark_result(T.matches12, n1);
      return RGBL_OK;
    }));
    RGBL_TRY(enqueue_triangulation(m, s, T, prm, sn.npairs()));
    RGBL_TRY(hc.fetch());
    memcpy(matches12, hc.host(T.matches12), sizeof(int32_t) * n1);
  }
  finish_matches12(sn, matches12, prm->check_orientation != 0, out_nmatches);
  return RGBL_OK;
}

namespace {
// What both new-point entries check before anything is queued.  chain: the search reads descriptors, mask and FeatureVector too.
int check_new_points_kf(const rgbl_matcher* m, const rgbl_new_points_keyframe* k, int n_levels, bool chain, const char* which) {
  if (!k) { set_error("%s: null key frame", which); return RGBL_ERR_INVALID; }
  const rgbl_keyframe_view& v = k->view;
  bool ok = v.n >= 0 && k->scale_factors && k->level_sigma2 && (v.n == 0 || k->depth);
  if (ok && v.device) ok = v.device->device == m->device && v.device->n == v.n;
  if (ok && !v.device && v.n > 0) ok = v.kp_xy && v.kp_octave && v.uright && (!chain || v.desc);
  if (ok && chain) ok = v.n_nodes >= 0 && (v.n == 0 || v.has_mappoint) && (v.n_nodes == 0 || (v.node_id && v.node_off && v.node_feat));
  if (!ok) { set_error("%s: invalid key frame (null array, negative count, or a resident frame of another size or device)", which); return RGBL_ERR_INVALID; }
  if (!v.device)
    for (int i = 0; i < v.n; ++i)
      if (v.kp_octave[i] < 0 || v.kp_octave[i] >= n_levels) { set_error("%s: octave %d of feature %d outside [0, %d)", which, v.kp_octave[i], i, n_levels); return RGBL_ERR_INVALID; }
  return RGBL_OK;
}
int check_new_points_params(const rgbl_new_points_params* p) {
  if (!p || p->n_levels < 1 || p->n_levels > kProjMaxLevels) { set_error("new points: n_levels outside [1, %d]", kProjMaxLevels); return RGBL_ERR_INVALID; }
  return RGBL_OK;
}
// inside the call's layout: the per-match block's arrays of one key frame (xy / oct / ur may already be there from the search's layout)
int put_new_points_kf(HostCall& hc, const rgbl_new_points_keyframe* k, int n_levels, bool features, NewPointsKf& d) {
  const rgbl_keyframe_view& v = k->view;
  if (features) RGBL_TRY(put_features(hc, v.device, v.n, nullptr, v.kp_xy, v.kp_octave, v.uright, nullptr, &d.xy, &d.oct, &d.ur));
  hc.put(&d.depth, k->depth, (size_t)v.n);
  if (k->kp_xy_raw) hc.put(&d.xy_raw, k->kp_xy_raw, (size_t)v.n * 2); else d.xy_raw = d.xy;
  hc.put(&d.scale, k->scale_factors, (size_t)n_levels);
  hc.put(&d.sigma2, k->level_sigma2, (size_t)n_levels);
  memcpy(d.Tcw, k->Tcw, sizeof(d.Tcw));
  memcpy(d.Ow, k->Ow, sizeof(d.Ow));
  memcpy(d.K, k->K, sizeof(d.K));
  d.mb = k->mb;
  return RGBL_OK;
}
NpParams new_points_params(const rgbl_new_points_keyframe* kf1, const rgbl_new_points_params* prm) {
  return NpParams{kf1->mbf, prm->ratio_factor, prm->th_far_points, prm->far_points, prm->inertial};
}
}  // namespace

int rgbl_triangulate_matches_host(const rgbl_new_points_keyframe* kf1, const rgbl_new_points_keyframe* kf2,
                                  const rgbl_new_points_params* prm, int n_pairs, const int32_t* idx1, const int32_t* idx2,
                                  rgbl_new_point* out) {
  if (!kf1 || !kf2 || !prm || n_pairs < 0 || (n_pairs > 0 && (!idx1 || !idx2 || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const NpParams P = new_points_params(kf1, prm);
  auto side = [&](const rgbl_new_points_keyframe* k, int i) {
    NpSide S;
    memcpy(S.Tcw, k->Tcw, sizeof(S.Tcw)); memcpy(S.Ow, k->Ow, sizeof(S.Ow)); memcpy(S.K, k->K, sizeof(S.K));
    S.mb = k->mb;
    const float* raw = k->kp_xy_raw ? k->kp_xy_raw : k->view.kp_xy;
    S.u = k->view.kp_xy[2 * i]; S.v = k->view.kp_xy[2 * i + 1]; S.u_raw = raw[2 * i]; S.v_raw = raw[2 * i + 1];
    S.uright = k->view.uright[i]; S.depth = k->depth[i];
    const int o = std::min(std::max(k->view.kp_octave[i], 0), prm->n_levels - 1);
    S.sigma2 = k->level_sigma2[o]; S.scale = k->scale_factors[o];
    return S;
  };
  for (int p = 0; p < n_pairs; ++p) {
    if (idx1[p] < 0 || idx1[p] >= kf1->view.n || idx2[p] < 0 || idx2[p] >= kf2->view.n) { set_error("pair %d: index out of range", p); return RGBL_ERR_INVALID; }
    rgbl_new_point r;
    memset(&r, 0, sizeof(r));
    r.idx1 = idx1[p]; r.idx2 = idx2[p];
    r.status = np_check(side(kf1, idx1[p]), side(kf2, idx2[p]), P, r.x3D);
    out[p] = r;
  }
  return RGBL_OK;
}

int rgbl_triangulate_matches(rgbl_matcher* m, const rgbl_new_points_keyframe* kf1, const rgbl_new_points_keyframe* kf2,
                             const rgbl_new_points_params* prm, int n_pairs, const int32_t* idx1, const int32_t* idx2,
                             rgbl_new_point* out) {
  if (!m || n_pairs < 0 || (n_pairs > 0 && (!idx1 || !idx2 || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(check_new_points_params(prm));
  RGBL_TRY(check_new_points_kf(m, kf1, prm->n_levels, false, "kf1"));
  RGBL_TRY(check_new_points_kf(m, kf2, prm->n_levels, false, "kf2"));
  for (int p = 0; p < n_pairs; ++p)
    if (idx1[p] < 0 || idx1[p] >= kf1->view.n || idx2[p] < 0 || idx2[p] >= kf2->view.n) { set_error("pair %d: index out of range", p); return RGBL_ERR_INVALID; }
  if (n_pairs == 0) return RGBL_OK;
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  NewPointsDev D;
  memset(&D, 0, sizeof(D));
  RGBL_TRY(hc.begin([&]() -> int {
    RGBL_TRY(put_new_points_kf(hc, kf1, prm->n_levels, true, D.k1));
    RGBL_TRY(put_new_points_kf(hc, kf2, prm->n_levels, true, D.k2));
    hc.put(&D.idx1, idx1, (size_t)n_pairs);
    const int32_t* d_idx2 = nullptr;
    hc.put(&d_idx2, idx2, (size_t)n_pairs);
    D.idx2 = const_cast<int32_t*>(d_idx2);
    D.total = hc.put_fill<int32_t>(3, 0);
    D.per_launch = D.total + 1;
    D.list = hc.scratch<int32_t>((size_t)n_pairs);
    D.out = hc.result<rgbl_new_point>((size_t)n_pairs);
    return RGBL_OK;
  }));
  D.P = new_points_params(kf1, prm);
  D.n = n_pairs; D.n_levels = prm->n_levels; D.report_rejected = 1; D.cap = n_pairs;
  RGBL_TRY(launch(m, s, "k_new_points", k_new_points, dim3(1), dim3(kNewPointsBS), 0, D));
  RGBL_TRY(hc.fetch());
  memcpy(out, hc.host(D.out), sizeof(rgbl_new_point) * (size_t)n_pairs);
  return RGBL_OK;
}

int rgbl_create_new_map_points(rgbl_matcher* m, const rgbl_new_points_keyframe* kf1, int n_neigh, const rgbl_new_points_keyframe* kf2,
                               const rgbl_triangulation_params* tri_prm, const uint8_t* skip, const rgbl_new_points_params* prm,
                               rgbl_new_point* out, int cap, int* n_out, int32_t* matches_per_neighbour, uint8_t* has_mappoint1_out) {
  if (!m || n_neigh < 0 || cap < 0 || !n_out || (cap > 0 && !out) || (n_neigh > 0 && (!kf2 || !tri_prm))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(check_new_points_params(prm));
  RGBL_TRY(check_new_points_kf(m, kf1, prm->n_levels, true, "kf1"));
  for (int i = 0; i < n_neigh; ++i) {
    RGBL_TRY(check_new_points_kf(m, kf2 + i, prm->n_levels, true, "kf2"));
    const rgbl_triangulation_params& t = tri_prm[i];
    if (t.check_orientation != 0) { set_error("neighbour %d: check_orientation has no form in the chain (LocalMapping.cc:412 passes false)", i); return RGBL_ERR_INVALID; }
    if (t.n_levels != prm->n_levels || !t.scale_factors2 || !t.level_sigma2_2) { set_error("neighbour %d: the search's level tables", i); return RGBL_ERR_INVALID; }
  }
  const int n1 = kf1->view.n;
  // which neighbours run (:444-460), and every merge walk (the searches' shared nodes) before the one upload
  std::vector<char> runs((size_t)n_neigh, 0);
  std::vector<SharedNodes> sn;
  sn.reserve((size_t)n_neigh);
  bool any = false;
  for (int i = 0; i < n_neigh; ++i) {
    sn.emplace_back(&kf1->view, &kf2[i].view);
    bool left_out = skip && skip[i];
    if (!left_out && !prm->monocular) {
      const float baseline = fr_norm(kf2[i].Ow[0] - kf1->Ow[0], kf2[i].Ow[1] - kf1->Ow[1], kf2[i].Ow[2] - kf1->Ow[2]);
      left_out = baseline < kf2[i].mb;
    }
    runs[i] = left_out ? 0 : (sn[i].empty() ? 1 : 2);   // 1: searched, nothing to launch; 2: launched
    any = any || runs[i] == 2;
  }
  int total = 0;
  std::vector<int32_t> per((size_t)n_neigh, 0);
  HostCall hc(m);
  uint8_t* d_mask = nullptr;
  rgbl_new_point* d_out = nullptr;
  if (any) {
    RGBL_HIP(hipSetDevice(m->device));
    StreamDrain drain(m->stream);  // error returns included
    hipStream_t s = hc.s;
    std::vector<TriDev> T((size_t)n_neigh);
    std::vector<NewPointsDev> D((size_t)n_neigh);
    TriDev T1;                 // key frame 1's side of every search
    NewPointsKf K1;
    int32_t *d_m12 = nullptr, *d_cnt = nullptr, *d_list = nullptr;
    RGBL_TRY(hc.begin([&]() -> int {
      RGBL_TRY(SharedNodes::put_first(hc, &kf1->view, {&T1.desc1, &T1.xy1, &K1.oct, &T1.ur1}, T1.fv));
      K1.xy = T1.xy1; K1.ur = T1.ur1;
      RGBL_TRY(put_new_points_kf(hc, kf1, prm->n_levels, false, K1));
      for (int i = 0; i < n_neigh; ++i) {
        if (runs[i] != 2) continue;
        memset(&D[i], 0, sizeof(D[i]));
        T[i] = T1;
        RGBL_TRY(sn[i].put_second(hc, {&T[i].desc2, &T[i].xy2, &T[i].oct2, &T[i].ur2}, T[i].fv));
        hc.put(&T[i].mp2, kf2[i].view.has_mappoint, (size_t)kf2[i].view.n);
        hc.put(&T[i].scale2, tri_prm[i].scale_factors2, (size_t)prm->n_levels);
        hc.put(&T[i].sigma2, tri_prm[i].level_sigma2_2, (size_t)prm->n_levels);
        D[i].k2.xy = T[i].xy2; D[i].k2.oct = T[i].oct2; D[i].k2.ur = T[i].ur2;
        RGBL_TRY(put_new_points_kf(hc, kf2 + i, prm->n_levels, false, D[i].k2));
      }
      d_m12 = hc.put_fill<int32_t>((size_t)n1, 0xff);   // all -1; k_new_points leaves it so for the next neighbour
      // what comes back, side by side: mask, counters, records
      const uint8_t* mask_up = nullptr;
      hc.put(&mask_up, kf1->view.has_mappoint, (size_t)n1);
      d_mask = const_cast<uint8_t*>(mask_up);
      hc.mark_result(d_mask, (size_t)n1);
      d_cnt = hc.put_fill<int32_t>((size_t)1 + 2 * (size_t)n_neigh, 0);
      hc.mark_result(d_cnt, (size_t)1 + 2 * (size_t)n_neigh);
      d_out = hc.result<rgbl_new_point>((size_t)cap);
      d_list = hc.scratch<int32_t>((size_t)n1);   // behind everything that travels
      return RGBL_OK;
    }));
    for (int i = 0; i < n_neigh; ++i) {
      if (runs[i] != 2) continue;
      T[i].mp1 = d_mask;
      T[i].matches12 = d_m12;
      RGBL_TRY(enqueue_triangulation(m, s, T[i], tri_prm + i, sn[i].npairs()));
      NewPointsDev& d = D[i];
      d.k1 = K1;
      d.P = new_points_params(kf1, prm);
      d.n = n1; d.n_levels = prm->n_levels;
      d.idx2 = d_m12; d.list = d_list; d.reset = 1; d.report_rejected = prm->report_rejected; d.neighbour = i; d.cap = cap;
      d.mask1 = d_mask; d.out = d_out; d.total = d_cnt; d.per_launch = d_cnt + 1 + 2 * i;
      RGBL_TRY(launch(m, s, "k_new_points", k_new_points, dim3(1), dim3(kNewPointsBS), 0, d));
    }
    RGBL_TRY(hc.fetch());
    const int32_t* cnt = hc.host(d_cnt);
    total = cnt[0];
    for (int i = 0; i < n_neigh; ++i) per[i] = cnt[1 + 2 * i];
  }
  *n_out = total;
  if (total > cap) { set_error("new points: %d records, room for %d", total, cap); return RGBL_ERR_CAPACITY; }
  if (total > 0) memcpy(out, hc.host(d_out), sizeof(rgbl_new_point) * (size_t)total);
  if (matches_per_neighbour)
    for (int i = 0; i < n_neigh; ++i) matches_per_neighbour[i] = runs[i] ? per[i] : -1;
  if (has_mappoint1_out && n1 > 0) {
    if (any) memcpy(has_mappoint1_out, hc.host(d_mask), (size_t)n1);
    else if (has_mappoint1_out != kf1->view.has_mappoint) memcpy(has_mappoint1_out, kf1->view.has_mappoint, (size_t)n1);
  }
  return RGBL_OK;
}

// test hooks for csrc/newpoint_math.h: Triangulate on the host, and the stereo parallax cosine on host and device
int rgbl_test_np_triangulate(const float* xn1, const float* xn2, const float* T1, const float* T2, float* x3D) {
  return np_triangulate(xn1, xn2, T1, T2, x3D) ? 1 : 0;
}
float rgbl_test_np_cos_parallax(float mb, float depth) { return np_cos_parallax_stereo(mb, depth); }
int rgbl_test_np_cos_parallax_device(float mb, const float* depth, float* y, int n) {
  if (!depth || !y || n < 1) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return elementwise_device_hook<float>({depth}, y, n, [&](float* const* d, float* dy, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_test_np_cos_parallax, grid, block, 0, 0, mb, (const float*)d[0], dy, n);
  });
}

// what the two greedy, best-only projection matchers (Frame-to-Frame and key-frame-to-Frame) hand to the kernels
namespace {
struct ProjHost {
  int n1, n2, n_levels;
  const uint8_t *valid1, *obs1 /* nullptr: every point blocks */, *mpdesc1, *desc2, *blocked2 /* nullable */;
  const float *wpos1, *angle1, *xy2, *angle2, *ur2 /* nullable */, *scale_factors;
  const int32_t *oct1, *oct2;
  const float *grid, *Tcw_q, *Tcw_t, *K;
  float mbf, th;
  int forward, backward, skip_behind, max_dist, check_orientation;
  int want_ur2;   // with dev2: the overload tests the stereo coordinate (ur2 is then the resident array)
  int sim3_mode;  // 0, or 1 / 2 = the projection form of the SearchByProjection(pKF, Scw, ...) overloads (wpos1 = camera-frame points)
  const rgbl_device_frame* dev2;  // nullable: the second frame's xy / octave / uright / descriptors resident on the device
};

// Frame::AssignFeaturesToGrid for the call: the resident frame's own grid when it has one for these image bounds
// (rgbl_device_frame_set_grid), else k_proj_grid on the call's scratch.  P.grid, P.xy2, P.blocked2 must be set.
void grid_for_call(rgbl_matcher* m, hipStream_t s, ProjDev& P, const rgbl_device_frame* dev2) {
  if (dev2 && dev2->has_grid && memcmp(dev2->grid, P.grid, sizeof(P.grid)) == 0) {
    P.cell_start = dev2->d_cell_start;
    P.cell_items = dev2->d_cell_items;
    P.init_taken = 1;
    return;
  }
  P.init_taken = 0;
  m->timer.begin("k_proj_grid", s);
  launch_proj_grid(P, s);
  m->timer.end(s);
}

// The greedy, best-only searches (SearchByProjection in three forms, SearchLocalPoints, SearchForInitialization): candidates
// per point, then ONE block that settles them in point order, in LDS when both sets fit.  greedy_layout() carves the result
// (P.choice) and the scratch inside the call's layout; greedy_search() launches.
struct GreedyKernels {
  void (*candidates)(ProjDev);
  void (*resolve_lds)(ProjDev);
  void (*resolve_global)(ProjDev);
  const char *candidates_name, *resolve_name;
};

void greedy_layout(HostCall& hc, ProjDev& P) {
  P.choice = hc.result<int32_t>(P.n1);
  P.cell_start = hc.scratch<uint32_t>(kGridCells + 1);
  P.cell_items = hc.scratch<uint16_t>(P.n2);
  P.taken_by = hc.scratch<int32_t>(P.n2);
  P.min_unres = hc.scratch<int32_t>(P.n2);
  P.win = hc.scratch<float4>(P.n1);
  P.rng = hc.scratch<int4>(P.n1);
  P.clist = hc.scratch<uint32_t>((size_t)P.n1 * kProjCand);
  P.cref = hc.scratch<uint32_t>(P.n1);
  P.state = hc.scratch<uint8_t>(P.n1);
}

// The entry points' shared argument tests and host passes.  sizes_ok: a feature's index travels in 16 bits, a level indexes P.scale.
bool sizes_ok(int n1, int n2, int n_levels) { return n1 >= 0 && n2 >= 0 && n2 <= 65535 && n_levels >= 1 && n_levels <= kProjMaxLevels; }
int check_point_count(int n1) {
  if (n1 < (1 << 20)) return RGBL_OK;
  set_error("at most 2^20 - 1 map points per call (a point's index travels in 20 bits of the resolve kernel's announcements)");
  return RGBL_ERR_INVALID;
}
// the levels of the points the call looks at index n_levels scale factors
int check_levels(const uint8_t* valid, const int32_t* level, int n, int n_levels, const char* what) {
  for (int i = 0; i < n; ++i)
    if (valid[i] && (level[i] < 0 || level[i] >= n_levels)) { set_error("%s", what); return RGBL_ERR_INVALID; }
  return RGBL_OK;
}
void set_scales(ProjDev& P, const float* factors, int n_levels) {
  for (int l = 0; l < kProjMaxLevels; ++l) P.scale[l] = l < n_levels ? factors[l] : 1.f;
}
// what the loop leaves in the frame's mvpMapPoints (a later point overwrites an unobserved earlier one); returns the match count
int scatter_matches(const int32_t* choice, int n1, int32_t* match2) {
  int nmatches = 0;
  for (int i = 0; i < n1; ++i)
    if (choice[i] >= 0) { match2[choice[i]] = i; ++nmatches; }
  return nmatches;
}

int greedy_search(rgbl_matcher* m, hipStream_t s, ProjDev& P, const rgbl_device_frame* dev2, const GreedyKernels& K) {
  grid_for_call(m, s, P, dev2);
  RGBL_TRY(launch(m, s, K.candidates_name, K.candidates, dim3((P.n1 + kPointsPerBlock - 1) / kPointsPerBlock), dim3(256), 0, P));
  const bool lds = P.n2 <= kResolveLdsN2 && P.n1 <= kResolveLdsN1;
  return launch(m, s, K.resolve_name, lds ? K.resolve_lds : K.resolve_global, dim3(1), dim3(kResolveBS), 0, P);
}

int projection_core(rgbl_matcher* m, const ProjHost& in, int32_t* match2, int* out_nmatches) {
  const int n1 = in.n1, n2 = in.n2;
  RGBL_TRY(check_point_count(n1));  // before anything is written: a refused call leaves the outputs as they were
  *out_nmatches = 0;
  for (int i = 0; i < n2; ++i) match2[i] = -1;
  if (n1 == 0 || n2 == 0) return RGBL_OK;
  RGBL_TRY(check_levels(in.valid1, in.oct1, n1, in.n_levels, "octave out of range"));
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  ProjDev P;
  P.n1 = n1; P.n2 = n2;
  P.proj1 = nullptr; P.level1 = nullptr; P.viewcos1 = nullptr; P.blocked2 = nullptr; P.ur2 = nullptr; P.nnratio = 0.f;
  const bool want_ur = in.ur2 != nullptr || (in.dev2 && in.want_ur2);
  RGBL_TRY(hc.begin([&]() -> int {
    hc.put(&P.valid1, in.valid1, (size_t)n1);
    if (in.obs1) hc.put(&P.obs1, in.obs1, (size_t)n1);
    else P.obs1 = hc.put_fill<uint8_t>(n1, 1);   // every point blocks
    hc.put(&P.wpos1, in.wpos1, (size_t)n1 * 3);
    hc.put(&P.mpdesc1, in.mpdesc1, (size_t)n1 * 32);
    hc.put(&P.oct1, in.oct1, (size_t)n1);
    RGBL_TRY(put_features(hc, in.dev2, n2, in.desc2, in.xy2, in.oct2, in.ur2, &P.desc2, &P.xy2, &P.oct2, want_ur ? &P.ur2 : nullptr));
    if (in.blocked2) hc.put(&P.blocked2, in.blocked2, (size_t)n2);
    greedy_layout(hc, P);
    return RGBL_OK;
  }));
  memcpy(P.grid, in.grid, sizeof(P.grid));
  memcpy(P.q, in.Tcw_q, sizeof(P.q));
  memcpy(P.t, in.Tcw_t, sizeof(P.t));
  memcpy(P.K, in.K, sizeof(P.K));
  P.mbf = in.mbf;
  P.th = in.th;
  set_scales(P, in.scale_factors, in.n_levels);
  P.forward = in.forward; P.backward = in.backward;
  P.skip_behind = in.skip_behind; P.max_dist = in.max_dist;
  P.sim3_mode = in.sim3_mode;
  RGBL_TRY(greedy_search(m, s, P, in.dev2, {k_proj_candidates, k_proj_resolve<true>, k_proj_resolve<false>, "k_proj_candidates", "k_proj_resolve"}));
  RGBL_TRY(hc.fetch());
  const int32_t* choice = hc.host(P.choice);
  // what the loop leaves in CurrentFrame.mvpMapPoints (a later point overwrites an unobserved earlier one), the match
  // count, and the rotation-consistency pass (ORBmatcher.cc:1768-1790, 1860-1884 / 1961-2006): one pass, so not scatter_matches
  int nmatches = 0;
  RotationFilter rf;
  for (int i = 0; i < n1; ++i) {
    const int c = choice[i];
    if (c < 0) continue;
    match2[c] = i;
    ++nmatches;
    if (in.check_orientation) rf.add(c, in.angle1[i], in.angle2[c]);
  }
  // a feature chosen twice is un-counted twice, as in the reference
  if (in.check_orientation) rf.drop_outliers([&](int c) { match2[c] = -1; --nmatches; });
  *out_nmatches = nmatches;
  return RGBL_OK;
}
}  // namespace

int rgbl_search_by_projection(rgbl_matcher* m, const rgbl_projection_input* in, int32_t* match2, int* out_nmatches) {
  if (!m || !in || !match2 || !out_nmatches || !sizes_ok(in->n1, in->n2, in->n_levels)) {
    set_error("invalid argument (CurrentFrame may hold at most 65535 features, %d pyramid levels)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  ProjHost h{};
  h.n1 = in->n1; h.n2 = in->n2; h.n_levels = in->n_levels;
  h.valid1 = in->valid1; h.obs1 = in->mp_observed1; h.mpdesc1 = in->mp_desc1; h.desc2 = in->desc2; h.blocked2 = nullptr;
  h.wpos1 = in->world_pos1; h.angle1 = in->angle1; h.xy2 = in->kp2_xy; h.angle2 = in->kp2_angle; h.ur2 = in->uright2;
  h.scale_factors = in->scale_factors; h.oct1 = in->octave1; h.oct2 = in->kp2_octave;
  h.grid = in->grid; h.Tcw_q = in->Tcw_q; h.Tcw_t = in->Tcw_t; h.K = in->K;
  h.mbf = in->mbf; h.th = in->th;
  {
    // bForward / bBackward (ORBmatcher.cc:1686-1694): tlc = Tlw * Tcw.inverse().translation(), Sophus / Eigen arithmetic
    const float qi[4] = {-in->Tcw_q[0], -in->Tcw_q[1], -in->Tcw_q[2], in->Tcw_q[3]};
    float wx, wy, wz, lx, ly, lz;
    quat_rotate(qi, -in->Tcw_t[0], -in->Tcw_t[1], -in->Tcw_t[2], &wx, &wy, &wz);
    quat_rotate(in->Tlw_q, wx, wy, wz, &lx, &ly, &lz);
    lz += in->Tlw_t[2];
    (void)lx; (void)ly;
    h.forward = (lz > in->mb && !in->mono) ? 1 : 0;
    h.backward = (-lz > in->mb && !in->mono) ? 1 : 0;
  }
  h.skip_behind = 1;
  h.max_dist = 100;  // TH_HIGH
  h.check_orientation = in->check_orientation;
  h.dev2 = in->device2; h.want_ur2 = 1;
  return projection_core(m, h, match2, out_nmatches);
}

// int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
// (src/ORBmatcher.cc:1889-2010): the same greedy best-only search; every matched feature is occupied for the points after it
// (CurrentFrame.mvpMapPoints[i2] != NULL, :1949-1950), as are the features that hold a map point on entry; levels
// [predicted - 1, predicted + 1], radius th * scale[predicted], no stereo-coordinate test and no test of the sign of the depth.
int rgbl_search_by_projection_keyframe(rgbl_matcher* m, const rgbl_keyframe_projection_input* in, int32_t* match2,
                                       int* out_nmatches) {
  if (!m || !in || !match2 || !out_nmatches || !sizes_ok(in->n1, in->n2, in->n_levels) || in->orb_dist < 0 || in->orb_dist > 255) {
    set_error("invalid argument (CurrentFrame may hold at most 65535 features, %d pyramid levels, ORBdist 0..255)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  ProjHost h{};
  h.n1 = in->n1; h.n2 = in->n2; h.n_levels = in->n_levels;
  h.valid1 = in->valid1; h.obs1 = nullptr; h.mpdesc1 = in->mp_desc1; h.desc2 = in->desc2; h.blocked2 = in->occupied2;
  h.wpos1 = in->world_pos1; h.angle1 = in->angle1; h.xy2 = in->kp2_xy; h.angle2 = in->kp2_angle; h.ur2 = nullptr;
  h.scale_factors = in->scale_factors; h.oct1 = in->level1; h.oct2 = in->kp2_octave;
  h.grid = in->grid; h.Tcw_q = in->Tcw_q; h.Tcw_t = in->Tcw_t; h.K = in->K;
  h.mbf = 0.f; h.th = in->th;
  h.forward = 0; h.backward = 0;  // levels predicted - 1 ... predicted + 1
  h.skip_behind = 0;
  h.max_dist = in->orb_dist;
  h.check_orientation = in->check_orientation;
  h.dev2 = in->device2; h.want_ur2 = 0;
  return projection_core(m, h, match2, out_nmatches);
}

int rgbl_distinctive_descriptors(rgbl_matcher* m, const uint8_t* desc, const int32_t* off, int n_points, int32_t* best) {
  if (!m || !off || !best || n_points < 0) { set_error("null argument"); return RGBL_ERR_INVALID; }
  if (n_points == 0) return RGBL_OK;
  const int total = off[n_points];
  for (int p = 0; p < n_points; ++p)
    if (off[p + 1] < off[p] || off[p + 1] - off[p] > 65535) { set_error("offsets must ascend, at most 65535 observations per point"); return RGBL_ERR_INVALID; }
  if (off[0] != 0 || (total > 0 && !desc)) { set_error("offsets start at 0; descriptors missing"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  const uint8_t* d_desc = nullptr;
  const int32_t* d_off = nullptr;
  int32_t* d_best = nullptr;
  RGBL_TRY(hc.begin([&]() -> int {
    if (total > 0) hc.put(&d_desc, desc, (size_t)total * 32);
    hc.put(&d_off, off, (size_t)n_points + 1);
    d_best = hc.result<int32_t>(n_points);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_distinctive", k_distinctive, dim3(n_points), dim3(64), 0, d_desc, d_off, d_best));
  RGBL_TRY(hc.fetch());
  memcpy(best, hc.host(d_best), sizeof(int32_t) * n_points);
  return RGBL_OK;
}

static int fuse_core(rgbl_matcher* m, const rgbl_fuse_input* in, int cam_frame, int proj_form, int chi2_gate, int max_dist,
                     int want_ur2, int32_t* best_idx, int32_t* best_dist) {
  if (!m || !in || !best_idx || !sizes_ok(in->n1, in->n2, in->n_levels)) {
    set_error("invalid argument (the key frame may hold at most 65535 features, %d pyramid levels)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  const int n1 = in->n1, n2 = in->n2;
  for (int i = 0; i < n1; ++i) { best_idx[i] = -1; if (best_dist) best_dist[i] = 256; }
  if (n1 == 0 || n2 == 0) return RGBL_OK;
  RGBL_TRY(check_levels(in->valid1, in->level1, n1, in->n_levels, "predicted level out of range"));
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  ProjDev P{};
  P.n1 = n1; P.n2 = n2;
  RGBL_TRY(hc.begin([&]() -> int {
    hc.put(&P.valid1, in->valid1, (size_t)n1);
    hc.put(&P.wpos1, in->world_pos1, (size_t)n1 * 3);
    hc.put(&P.mpdesc1, in->mp_desc1, (size_t)n1 * 32);
    hc.put(&P.oct1, in->level1, (size_t)n1);
    RGBL_TRY(put_features(hc, in->device2, n2, in->desc2, in->kp2_xy, in->kp2_octave, in->uright2, &P.desc2, &P.xy2, &P.oct2,
                          want_ur2 ? &P.ur2 : nullptr));
    P.cand = hc.result<unsigned long long>(n1);
    P.cell_start = hc.scratch<uint32_t>(kGridCells + 1);
    P.cell_items = hc.scratch<uint16_t>(n2);
    P.taken_by = hc.scratch<int32_t>(n2);  // written by k_proj_grid, not used by the fuse search
    return RGBL_OK;
  }));
  memcpy(P.grid, in->grid, sizeof(P.grid));
  memcpy(P.q, in->Tcw_q, sizeof(P.q));
  memcpy(P.t, in->Tcw_t, sizeof(P.t));
  memcpy(P.K, in->K, sizeof(P.K));
  P.mbf = in->bf;
  P.th = in->th;
  FuseDev Fz;
  Fz.cam_frame = cam_frame; Fz.proj_form = proj_form; Fz.chi2_gate = chi2_gate;
  set_scales(P, in->scale_factors, in->n_levels);
  for (int l = 0; l < kProjMaxLevels; ++l) Fz.inv_sigma2[l] = l < in->n_levels ? in->inv_level_sigma2[l] : 1.f;
  grid_for_call(m, s, P, in->device2);
  RGBL_TRY(launch(m, s, "k_fuse_search", k_fuse_search, dim3((n1 + kPointsPerBlock - 1) / kPointsPerBlock), dim3(256), 0, P, Fz));
  RGBL_TRY(hc.fetch());
  const unsigned long long* keys = hc.host(P.cand);
  for (int i = 0; i < n1; ++i) {
    if (keys[i] == ~0ull) continue;
    const int dist = (int)(keys[i] >> 32);
    if (best_dist) best_dist[i] = dist;
    if (dist <= max_dist) best_idx[i] = (int)(keys[i] & 0xffffu);
  }
  return RGBL_OK;
}

// int ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints, vector<MapPoint*>&
// vpMatched, int th, float ratioHamming) (src/ORBmatcher.cc:427-532) and its overload with vpPointsKFs / vpMatchedKF (:534-646):
// the greedy best-only search again - a matched feature (vpMatched[idx] != NULL, on entry or set by an earlier point) is
// skipped by the points after it - on camera-frame points.
int rgbl_search_by_projection_sim3(rgbl_matcher* m, const rgbl_project_search_input* in, const uint8_t* matched2, int32_t* match2,
                                   int* out_nmatches) {
  if (!m || !in || !match2 || !out_nmatches || !sizes_ok(in->n1, in->n2, in->n_levels) || (in->proj_form != 0 && in->proj_form != 2) ||
      in->max_dist < 0 || in->max_dist > 255) {
    set_error("invalid argument (at most 65535 features, %d pyramid levels, proj_form 0 / 2, max_dist 0..255)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  const float ident_q[4] = {0.f, 0.f, 0.f, 1.f}, zero_t[3] = {0.f, 0.f, 0.f};
  ProjHost h{};
  h.n1 = in->n1; h.n2 = in->n2; h.n_levels = in->n_levels;
  h.valid1 = in->valid1; h.obs1 = nullptr; h.mpdesc1 = in->mp_desc1; h.desc2 = in->desc2; h.blocked2 = matched2;
  h.wpos1 = in->cam_pos1; h.angle1 = nullptr; h.xy2 = in->kp2_xy; h.angle2 = nullptr; h.ur2 = nullptr;
  h.scale_factors = in->scale_factors; h.oct1 = in->level1; h.oct2 = in->kp2_octave;
  h.grid = in->grid; h.Tcw_q = ident_q; h.Tcw_t = zero_t; h.K = in->K;
  h.mbf = 0.f; h.th = in->th;
  h.forward = 0; h.backward = 0; h.skip_behind = 0;
  h.max_dist = in->max_dist;
  h.check_orientation = 0;
  h.sim3_mode = in->proj_form == 0 ? 1 : 2;
  h.dev2 = in->device2; h.want_ur2 = 0;
  return projection_core(m, h, match2, out_nmatches);
}

int rgbl_fuse_search(rgbl_matcher* m, const rgbl_fuse_input* in, int32_t* best_idx, int32_t* best_dist) {
  return fuse_core(m, in, 0, 0, 1, 50 /* TH_LOW */, (in && (in->uright2 || in->device2)) ? 1 : 0, best_idx, best_dist);
}

// The per-point search shared by ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1340-1455:
// Pinhole::project, best <= TH_LOW) and by both directions of SearchBySim3 (:1457-1674: invz = 1.0 / z, best <= TH_HIGH): the
// caller has already moved the points into the key frame's camera frame with its SE3 / Sim3 objects.
int rgbl_project_search(rgbl_matcher* m, const rgbl_project_search_input* in, int32_t* best_idx, int32_t* best_dist) {
  if (!in || (in->proj_form != 0 && in->proj_form != 1) || in->max_dist < 0 || in->max_dist > 255) {
    set_error("invalid argument (proj_form 0 / 1, max_dist 0..255)");
    return RGBL_ERR_INVALID;
  }
  rgbl_fuse_input f{};
  f.n1 = in->n1; f.valid1 = in->valid1; f.world_pos1 = in->cam_pos1; f.mp_desc1 = in->mp_desc1; f.level1 = in->level1;
  f.n2 = in->n2; f.kp2_xy = in->kp2_xy; f.kp2_octave = in->kp2_octave; f.uright2 = nullptr; f.desc2 = in->desc2;
  memcpy(f.grid, in->grid, sizeof(f.grid));
  f.Tcw_q[3] = 1.f;
  memcpy(f.K, in->K, sizeof(f.K));
  f.bf = 0.f;
  f.scale_factors = in->scale_factors;
  f.inv_level_sigma2 = in->scale_factors;  // not read without the chi-square gate
  f.n_levels = in->n_levels;
  f.th = in->th;
  f.device2 = in->device2;
  return fuse_core(m, &f, 1, in->proj_form, 0, in->max_dist, 0, best_idx, best_dist);
}

int rgbl_search_local_points(rgbl_matcher* m, const rgbl_local_points_input* in, int32_t* match2, int* out_nmatches) {
  if (!m || !in || !match2 || !out_nmatches || !sizes_ok(in->n1, in->n2, in->n_levels)) {
    set_error("invalid argument (the frame may hold at most 65535 features, %d pyramid levels)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  RGBL_TRY(check_point_count(in->n1));
  *out_nmatches = 0;
  const int n1 = in->n1, n2 = in->n2;
  for (int i = 0; i < n2; ++i) match2[i] = -1;
  if (n1 == 0 || n2 == 0) return RGBL_OK;
  RGBL_TRY(check_levels(in->valid1, in->level1, n1, in->n_levels, "predicted level out of range"));
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  ProjDev P;
  memset(&P, 0, sizeof(P));
  P.n1 = n1; P.n2 = n2;
  RGBL_TRY(hc.begin([&]() -> int {
    hc.put(&P.valid1, in->valid1, (size_t)n1);
    hc.put(&P.obs1, in->mp_observed1, (size_t)n1);
    hc.put(&P.proj1, in->proj1, (size_t)n1 * 3);
    hc.put(&P.mpdesc1, in->mp_desc1, (size_t)n1 * 32);
    hc.put(&P.level1, in->level1, (size_t)n1);
    hc.put(&P.viewcos1, in->view_cos1, (size_t)n1);
    RGBL_TRY(put_features(hc, in->device2, n2, in->desc2, in->kp2_xy, in->kp2_octave, in->uright2, &P.desc2, &P.xy2, &P.oct2, &P.ur2));
    if (in->blocked2) hc.put(&P.blocked2, in->blocked2, (size_t)n2);
    greedy_layout(hc, P);
    return RGBL_OK;
  }));
  memcpy(P.grid, in->grid, sizeof(P.grid));
  P.th = in->th;
  P.nnratio = in->nnratio;
  set_scales(P, in->scale_factors, in->n_levels);
  RGBL_TRY(greedy_search(m, s, P, in->device2, {k_local_candidates, k_local_resolve<true>, k_local_resolve<false>, "k_local_candidates", "k_local_resolve"}));
  RGBL_TRY(hc.fetch());
  *out_nmatches = scatter_matches(hc.host(P.choice), n1, match2);
  return RGBL_OK;
}

namespace {
constexpr int kMaxPoolSlots = 1 << 26;   // 4 GiB of slots: keeps every byte offset far inside size_t / int arithmetic
struct PoolArrays { size_t wpos, normal, min_d, max_d, desc, total; };
PoolArrays pool_arrays(int cap) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  PoolArrays a;
  a.wpos = 0;
  a.normal = up(a.wpos + (size_t)cap * 12);
  a.min_d = up(a.normal + (size_t)cap * 12);
  a.max_d = up(a.min_d + (size_t)cap * 4);
  a.desc = up(a.max_d + (size_t)cap * 4);
  a.total = up(a.desc + (size_t)cap * 32);
  return a;
}
// a zeroed block for `cap` slots with the first `keep` slots of the pool's present arrays copied over; replaces the old block
int pool_resize(rgbl_map_points* p, int cap, int keep) {
  const PoolArrays a = pool_arrays(cap);
  uint8_t* nb = nullptr;
  RGBL_HIP(rgbl::device_alloc(reinterpret_cast<void**>(&nb), a.total));
  hipError_t e = hipMemset(nb, 0, a.total);
  if (e == hipSuccess && keep > 0) {
    const struct { size_t off; const void* src; size_t bytes; } part[5] = {
        {a.wpos, p->d_wpos, (size_t)keep * 12}, {a.normal, p->d_normal, (size_t)keep * 12}, {a.min_d, p->d_min, (size_t)keep * 4},
        {a.max_d, p->d_max, (size_t)keep * 4}, {a.desc, p->d_desc, (size_t)keep * 32}};
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMemcpy(nb + part[k].off, part[k].src, part[k].bytes, hipMemcpyDeviceToDevice);
  }
  // the matcher streams that read the block next are non-blocking or the caller's: nothing above is left in flight
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(nb); set_error("map point pool: %s", hipGetErrorString(e)); return RGBL_ERR_HIP; }
  if (p->block) (void)hipFree(p->block);
  p->block = nb; p->cap = cap;
  p->d_wpos = reinterpret_cast<float*>(nb + a.wpos); p->d_normal = reinterpret_cast<float*>(nb + a.normal);
  p->d_min = reinterpret_cast<float*>(nb + a.min_d); p->d_max = reinterpret_cast<float*>(nb + a.max_d);
  p->d_desc = nb + a.desc;
  return RGBL_OK;
}
}  // namespace

int rgbl_map_points_create(int device, int capacity, rgbl_map_points** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (capacity < 1 || capacity > kMaxPoolSlots) { set_error("map point pool: capacity 1 .. %d", kMaxPoolSlots); return RGBL_ERR_INVALID; }
  if (rgbl_device_count() <= device || device < 0) {
    set_error("no usable HIP device %d (this library has no CPU fallback)", device);
    return RGBL_ERR_NO_DEVICE;
  }
  RGBL_HIP(hipSetDevice(device));
  rgbl_map_points* p = new rgbl_map_points;
  p->device = device;
  int rc = pool_resize(p, capacity, 0);
  if (rc == RGBL_OK && hipStreamCreate(&p->stream) != hipSuccess) { set_error("hipStreamCreate failed"); rc = RGBL_ERR_HIP; }
  if (rc != RGBL_OK) { if (p->block) (void)hipFree(p->block); delete p; return rc; }
  *out = p;
  return RGBL_OK;
}

void rgbl_map_points_destroy(rgbl_map_points* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  { std::lock_guard<std::mutex> lock(p->mu); (void)hipStreamSynchronize(p->stream); }
  if (p->block) (void)hipFree(p->block);
  if (p->d_stage) (void)hipFree(p->d_stage);
  if (p->h_stage) (void)hipHostFree(p->h_stage);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
}

int rgbl_map_points_capacity(rgbl_map_points* p) {
  if (!p) return 0;
  std::lock_guard<std::mutex> lock(p->mu);
  return p->cap;
}

int rgbl_map_points_reserve(rgbl_map_points* p, int capacity) {
  if (!p || capacity < 1 || capacity > kMaxPoolSlots) { set_error("map point pool: capacity 1 .. %d", kMaxPoolSlots); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(p->mu);
  if (capacity <= p->cap) return RGBL_OK;
  RGBL_HIP(hipSetDevice(p->device));
  return pool_resize(p, capacity, p->cap);
}

int rgbl_map_points_update(rgbl_map_points* p, int n, const int32_t* slot, const float* world_pos, const float* normal,
                           const float* min_dist, const float* max_dist, const uint8_t* desc) {
  if (!p || n < 0 || (n > 0 && !slot)) { set_error("null argument"); return RGBL_ERR_INVALID; }
  if (n == 0) return RGBL_OK;
  std::lock_guard<std::mutex> lock(p->mu);
  for (int k = 0; k < n; ++k)
    if (slot[k] < 0 || slot[k] >= p->cap) { set_error("map point pool: slot %d outside [0, %d)", slot[k], p->cap); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(p->device));
  // the packed arrays, 256-byte aligned: slot | world_pos | normal | min | max | desc (only the ones given)
  size_t off = 0;
  auto take = [&](size_t bytes, bool present) { off = (off + 255) / 256 * 256; const size_t o = off; if (present) off += bytes; return o; };
  const size_t o_slot = take((size_t)n * 4, true), o_wpos = take((size_t)n * 12, world_pos), o_normal = take((size_t)n * 12, normal),
               o_min = take((size_t)n * 4, min_dist), o_max = take((size_t)n * 4, max_dist), o_desc = take((size_t)n * 32, desc);
  if (off > p->stage_size) {
    if (p->d_stage) { (void)hipFree(p->d_stage); p->d_stage = nullptr; }
    if (p->h_stage) { (void)hipHostFree(p->h_stage); p->h_stage = nullptr; }
    p->stage_size = 0;
    const size_t sz = std::max(off, (size_t)1 << 16);
    RGBL_HIP(rgbl::device_alloc(reinterpret_cast<void**>(&p->d_stage), sz));
    RGBL_HIP(rgbl::pinned_alloc(&p->h_stage, sz));
    p->stage_size = sz;
  }
  RGBL_HIP(refill_staging(p->d_stage, p->h_stage, off, p->stream));
  int32_t* h_slot = reinterpret_cast<int32_t*>(p->h_stage + o_slot);
  memcpy(h_slot, slot, (size_t)n * 4);
  {  // a slot listed more than once keeps its last entry: the earlier ones are struck out, so no two work-items write one slot
    std::vector<std::pair<int32_t, int32_t>> order((size_t)n);
    for (int k = 0; k < n; ++k) order[(size_t)k] = {slot[k], k};
    std::sort(order.begin(), order.end());
    for (int k = 0; k + 1 < n; ++k)
      if (order[(size_t)k].first == order[(size_t)k + 1].first) h_slot[order[(size_t)k].second] = -1;
  }
  if (world_pos) memcpy(p->h_stage + o_wpos, world_pos, (size_t)n * 12);
  if (normal) memcpy(p->h_stage + o_normal, normal, (size_t)n * 12);
  if (min_dist) memcpy(p->h_stage + o_min, min_dist, (size_t)n * 4);
  if (max_dist) memcpy(p->h_stage + o_max, max_dist, (size_t)n * 4);
  if (desc) memcpy(p->h_stage + o_desc, desc, (size_t)n * 32);
  StreamDrain drain(p->stream);
  RGBL_HIP(hipMemcpyAsync(p->d_stage, p->h_stage, off, hipMemcpyHostToDevice, p->stream));
  PoolScatter S{};
  S.n = n;
  S.slot = reinterpret_cast<const int32_t*>(p->d_stage + o_slot);
  S.wpos = world_pos ? reinterpret_cast<const float*>(p->d_stage + o_wpos) : nullptr;
  S.normal = normal ? reinterpret_cast<const float*>(p->d_stage + o_normal) : nullptr;
  S.min_dist = min_dist ? reinterpret_cast<const float*>(p->d_stage + o_min) : nullptr;
  S.max_dist = max_dist ? reinterpret_cast<const float*>(p->d_stage + o_max) : nullptr;
  S.desc = desc ? p->d_stage + o_desc : nullptr;
  S.p_wpos = p->d_wpos; S.p_normal = p->d_normal; S.p_min = p->d_min; S.p_max = p->d_max; S.p_desc = p->d_desc;
  hipLaunchKernelGGL(k_map_points_scatter, dim3((n + 255) / 256), dim3(256), 0, p->stream, S);
  RGBL_HIP(hipGetLastError());
  RGBL_HIP(hipStreamSynchronize(p->stream));
  return RGBL_OK;
}

int rgbl_map_points_download(rgbl_map_points* p, int n, const int32_t* slot, float* world_pos, float* normal, float* min_dist,
                             float* max_dist, uint8_t* desc) {
  if (!p || n < 0 || (n > 0 && !slot)) { set_error("null argument"); return RGBL_ERR_INVALID; }
  if (n == 0) return RGBL_OK;
  std::lock_guard<std::mutex> lock(p->mu);
  int lo = p->cap, hi = -1;
  for (int k = 0; k < n; ++k) {
    if (slot[k] < 0 || slot[k] >= p->cap) { set_error("map point pool: slot %d outside [0, %d)", slot[k], p->cap); return RGBL_ERR_INVALID; }
    lo = std::min(lo, slot[k]); hi = std::max(hi, slot[k]);
  }
  RGBL_HIP(hipSetDevice(p->device));
  // the slots between the lowest and the highest one listed, one copy per array
  const size_t span = (size_t)(hi - lo) + 1;
  std::vector<uint8_t> buf(span * 32);
  const struct { const void* src; void* dst; size_t per; } part[5] = {
      {p->d_wpos, world_pos, 12}, {p->d_normal, normal, 12}, {p->d_min, min_dist, 4}, {p->d_max, max_dist, 4}, {p->d_desc, desc, 32}};
  for (int a = 0; a < 5; ++a) {
    if (!part[a].dst) continue;
    const size_t per = part[a].per;
    RGBL_HIP(hipMemcpy(buf.data(), static_cast<const uint8_t*>(part[a].src) + (size_t)lo * per, span * per, hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) memcpy(static_cast<uint8_t*>(part[a].dst) + (size_t)k * per, buf.data() + (size_t)(slot[k] - lo) * per, per);
  }
  return RGBL_OK;
}

// MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors for pool slots (include/rgbl_frontend.h).
// Everything is checked on the host before the first launch: the kernels index with the caller's numbers.
int rgbl_map_points_refresh(rgbl_matcher* m, rgbl_map_points* pool, const rgbl_map_refresh_input* in, rgbl_map_refresh_output* out) {
  if (!m || !pool || !in || in->n_points < 0) { set_error("null argument"); return RGBL_ERR_INVALID; }
  const int np = in->n_points, nk = in->n_kfs;
  if (np == 0) return RGBL_OK;
  const bool do_n = in->do_normal != 0, do_d = in->do_descriptor != 0;
  if (np > (1 << 24) || !in->slot || !in->obs_off || in->obs_off[0] != 0 || nk < 0) { set_error("map refresh: 1 .. 2^24 points with slots and offsets that start at 0"); return RGBL_ERR_INVALID; }
  if (pool->device != m->device) { set_error("map refresh: the pool is on device %d, the matcher on %d", pool->device, m->device); return RGBL_ERR_INVALID; }
  for (int p = 0; p < np; ++p)
    if (in->obs_off[p + 1] < in->obs_off[p] || in->obs_off[p + 1] - in->obs_off[p] > 65535) { set_error("map refresh: offsets must ascend, at most 65535 observations per point"); return RGBL_ERR_INVALID; }
  const int total = in->obs_off[np];
  if ((total > 0 && (!in->obs_kf || !in->obs_feat)) || (nk > 0 && ((do_n && !in->kf_center) || (do_d && !in->kf_frame)))) { set_error("map refresh: null argument"); return RGBL_ERR_INVALID; }
  if (do_n) {
    if (in->n_levels < 1 || in->n_levels > kProjMaxLevels || !in->scale_factors || !in->ref_kf || !in->ref_level) { set_error("map refresh: 1 .. %d pyramid levels with their scale factors, a reference key frame and level per point", kProjMaxLevels); return RGBL_ERR_INVALID; }
    for (int p = 0; p < np; ++p) {
      if (in->ref_kf[p] < 0 || in->ref_kf[p] >= nk) { set_error("map refresh: reference key frame %d of point %d outside [0, %d)", in->ref_kf[p], p, nk); return RGBL_ERR_INVALID; }
      if (in->ref_level[p] < 0 || in->ref_level[p] >= in->n_levels) { set_error("map refresh: reference level %d of point %d outside [0, %d)", in->ref_level[p], p, in->n_levels); return RGBL_ERR_INVALID; }
    }
  }
  for (int k = 0; k < nk; ++k) {
    const rgbl_device_frame* f = in->kf_frame ? in->kf_frame[k] : nullptr;
    if (do_d && !f) { set_error("map refresh: key frame %d is not resident on the device", k); return RGBL_ERR_INVALID; }
    if (f && f->device != m->device) { set_error("map refresh: key frame %d is on device %d, the matcher on %d", k, f->device, m->device); return RGBL_ERR_INVALID; }
  }
  std::vector<uint8_t> observed((size_t)nk, 0);   // the key frames some observation names: the ones the stream waits for
  for (int o = 0; o < total; ++o) {
    const int kf = in->obs_kf[o];
    if (kf >= 0 && kf < nk) observed[(size_t)kf] = 1;
    if (kf < 0 || kf >= nk) { set_error("map refresh: observation %d names key frame %d outside [0, %d)", o, kf, nk); return RGBL_ERR_INVALID; }
    const rgbl_device_frame* f = in->kf_frame ? in->kf_frame[kf] : nullptr;
    if (f && (in->obs_feat[o] < 0 || in->obs_feat[o] >= f->n)) { set_error("map refresh: observation %d names feature %d of a key frame with %d", o, in->obs_feat[o], f->n); return RGBL_ERR_INVALID; }
  }
  // rows per point (the observations of key frames that are not bad); the lists too long for LDS get room in the scratch
  std::vector<int32_t> long_off;
  size_t long_rows = 0;
  if (do_d) {
    long_off.assign((size_t)np, -1);
    for (int p = 0; p < np; ++p) {
      int rows = 0;
      for (int o = in->obs_off[p]; o < in->obs_off[p + 1]; ++o) rows += !(in->kf_bad && in->kf_bad[in->obs_kf[o]]);
      if (rows > kRefreshLdsRows) { long_off[(size_t)p] = (int32_t)long_rows; long_rows += (size_t)rows; }
    }
    if (long_rows > (size_t)INT_MAX) { set_error("map refresh: too many observations"); return RGBL_ERR_INVALID; }
  }
  std::lock_guard<std::mutex> pool_lock(pool->mu);
  {
    std::vector<int32_t> sorted(in->slot, in->slot + np);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= pool->cap) { set_error("map point pool: slot %d outside [0, %d)", sorted.front() < 0 ? sorted.front() : sorted.back(), pool->cap); return RGBL_ERR_INVALID; }
    for (int p = 0; p + 1 < np; ++p)
      if (sorted[(size_t)p] == sorted[(size_t)p + 1]) { set_error("map refresh: slot %d is listed twice", sorted[(size_t)p]); return RGBL_ERR_INVALID; }
  }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included; declared behind pool_lock: the stream is drained before the pool is released
  HostCall hc(m);
  hipStream_t s = hc.s;
  RefreshDev R;
  memset(&R, 0, sizeof(R));
  const float* d_wpos = nullptr;
  const bool want_n = out && (out->normal || out->min_dist || out->max_dist), want_d = out && out->desc;
  const bool run_n = do_n || want_n, run_d = do_d || want_d;
  uint8_t *wrote_n = nullptr, *wrote_d = nullptr;
  RGBL_TRY(hc.begin([&]() -> int {
    hc.put(&R.slot, in->slot, (size_t)np);
    hc.put(&R.off, in->obs_off, (size_t)np + 1);
    if (in->world_pos) hc.put(&d_wpos, in->world_pos, (size_t)np * 3);
    if (do_n || do_d) hc.put(&R.obs_kf, in->obs_kf, (size_t)total);
    if (do_n) {
      hc.put(&R.ref_kf, in->ref_kf, (size_t)np);
      hc.put(&R.ref_level, in->ref_level, (size_t)np);
      hc.put(&R.kf_center, in->kf_center, (size_t)nk * 3);
      hc.put(&R.scale, in->scale_factors, (size_t)in->n_levels);
    }
    if (do_d) {
      hc.put(&R.obs_feat, in->obs_feat, (size_t)total);
      hc.put(&R.long_off, (const int32_t*)long_off.data(), (size_t)np);
      if (in->kf_bad) hc.put(&R.kf_bad, in->kf_bad, (size_t)nk);
      else R.kf_bad = hc.put_fill<uint8_t>((size_t)nk, 0);
      R.kf_desc = hc.stage<const uint8_t*>((size_t)nk, [&](const uint8_t** t) { for (int k = 0; k < nk; ++k) t[k] = in->kf_frame[k]->d_desc; });
      if (hc.carving)   // the stream waits for whatever filled the observed key frames last
        for (int k = 0; k < nk; ++k)
          if (observed[(size_t)k]) RGBL_HIP(hipStreamWaitEvent(s, in->kf_frame[k]->ready, 0));
      R.rows = hc.scratch<unsigned long long>(long_rows * 4);
    }
    if (out) {   // the results back to back: one copy back
      if (out->normal) R.o_normal = hc.result<float>((size_t)np * 3);
      if (out->min_dist) R.o_min = hc.result<float>((size_t)np);
      if (out->max_dist) R.o_max = hc.result<float>((size_t)np);
      if (out->best_obs && do_d) R.o_best = hc.result<int32_t>((size_t)np);
      if (out->desc) R.o_desc = hc.result<uint8_t>((size_t)np * 32);
      if (out->status && run_n) wrote_n = hc.result<uint8_t>((size_t)np);
      if (out->status && run_d) wrote_d = hc.result<uint8_t>((size_t)np);
    }
    return RGBL_OK;
  }));
  R.p_wpos = pool->d_wpos; R.p_normal = pool->d_normal; R.p_min = pool->d_min; R.p_max = pool->d_max; R.p_desc = pool->d_desc;
  if (in->world_pos) {   // SetWorldPos first: the kernels below read the new positions
    PoolScatter S{};
    S.n = np; S.slot = R.slot; S.wpos = d_wpos;
    S.p_wpos = pool->d_wpos; S.p_normal = pool->d_normal; S.p_min = pool->d_min; S.p_max = pool->d_max; S.p_desc = pool->d_desc;
    RGBL_TRY(launch(m, s, "k_map_points_scatter", k_map_points_scatter, dim3((np + 255) / 256), dim3(256), 0, S));
  }
  if (run_n) {
    if (do_n) R.top_scale = in->scale_factors[in->n_levels - 1];
    R.compute = do_n; R.o_wrote = wrote_n;
    RGBL_TRY(launch(m, s, "k_map_refresh_normal", k_map_refresh_normal, dim3(np), dim3(64), 0, R));
  }
  if (run_d) {
    R.compute = do_d; R.o_wrote = wrote_d;
    RGBL_TRY(launch(m, s, "k_map_refresh_desc", k_map_refresh_desc, dim3(np), dim3(64), 0, R));
  }
  RGBL_TRY(hc.fetch());
  if (out) {
    if (out->normal) memcpy(out->normal, hc.host(R.o_normal), sizeof(float) * 3 * (size_t)np);
    if (out->min_dist) memcpy(out->min_dist, hc.host(R.o_min), sizeof(float) * (size_t)np);
    if (out->max_dist) memcpy(out->max_dist, hc.host(R.o_max), sizeof(float) * (size_t)np);
    if (out->best_obs) {
      if (R.o_best) memcpy(out->best_obs, hc.host(R.o_best), sizeof(int32_t) * (size_t)np);
      else for (int p = 0; p < np; ++p) out->best_obs[p] = -1;
    }
    if (out->desc) memcpy(out->desc, hc.host(R.o_desc), (size_t)np * 32);
    if (out->status)
      for (int p = 0; p < np; ++p)
        out->status[p] = (uint8_t)((wrote_n ? hc.host(wrote_n)[p] : 0) | (wrote_d ? hc.host(wrote_d)[p] << 1 : 0));
  }
  return RGBL_OK;
}

// Tracking::SearchLocalPoints from its second loop on (Tracking.cc:3399-3448): k_frustum, and behind it - on the arrays it
// left in the call's scratch - the kernels of rgbl_search_local_points, unchanged.
namespace {
int track_local_core(rgbl_matcher* m, const rgbl_track_local_input* in, uint8_t* in_view, rgbl_frustum_record* rec, int* n_in_view,
                     bool search, int32_t* match2, int* out_nmatches) {
  if (!m || !in || !n_in_view || !sizes_ok(in->n1, search ? in->n2 : 0, in->n_levels) || (in->n1 > 0 && !in_view) ||
      (search && (!match2 || !out_nmatches))) {
    set_error("invalid argument (the frame may hold at most 65535 features, %d pyramid levels)", kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  RGBL_TRY(check_point_count(in->n1));
  const int n1 = in->n1, n2 = search ? in->n2 : 0;
  *n_in_view = 0;
  if (search) {
    *out_nmatches = 0;
    for (int i = 0; i < n2; ++i) match2[i] = -1;
  }
  if (n1 == 0) return RGBL_OK;
  const bool do_search = search && n2 > 0;
  rgbl_map_points* pool = in->pool;
  if (pool ? (!in->slot1 || pool->device != m->device)
           : (!in->world_pos1 || !in->normal1 || !in->min_dist1 || !in->max_dist1 || (do_search && !in->mp_desc1))) {
    set_error("map points: either host arrays (world_pos1, normal1, min_dist1, max_dist1, mp_desc1) or a pool on the matcher's device with slot1");
    return RGBL_ERR_INVALID;
  }
  if (do_search && !in->mp_observed1) { set_error("null argument"); return RGBL_ERR_INVALID; }
  const rgbl_frustum_record none = {-1.f, -1.f, 0.f, 0.f, 0.f, 0};
  bool any = !in->consider1;
  for (int i = 0; i < n1 && !any; ++i) any = in->consider1[i] != 0;
  if (!any) {   // nothing to project: what isInFrustum would have left is known here
    memset(in_view, 0, (size_t)n1);
    if (rec) for (int i = 0; i < n1; ++i) rec[i] = none;
    return RGBL_OK;
  }
  std::unique_lock<std::mutex> pool_lock;
  if (pool) {
    pool_lock = std::unique_lock<std::mutex>(pool->mu);
    for (int i = 0; i < n1; ++i)
      if (in->slot1[i] < 0 || in->slot1[i] >= pool->cap) { set_error("map point pool: slot %d outside [0, %d)", in->slot1[i], pool->cap); return RGBL_ERR_INVALID; }
  }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included; declared behind pool_lock: the stream is drained before the pool is released
  HostCall hc(m);
  hipStream_t s = hc.s;
  FrustumDev F;
  memset(&F, 0, sizeof(F));
  ProjDev P;
  memset(&P, 0, sizeof(P));
  F.n1 = n1; P.n1 = n1; P.n2 = n2;
  RGBL_TRY(hc.begin([&]() -> int {
    if (in->consider1) hc.put(&F.consider1, in->consider1, (size_t)n1);
    if (pool) {
      hc.put(&F.slot1, in->slot1, (size_t)n1);
      F.wpos = pool->d_wpos; F.normal = pool->d_normal; F.min_dist = pool->d_min; F.max_dist = pool->d_max; F.desc = pool->d_desc;
    } else {
      hc.put(&F.wpos, in->world_pos1, (size_t)n1 * 3);
      hc.put(&F.normal, in->normal1, (size_t)n1 * 3);
      hc.put(&F.min_dist, in->min_dist1, (size_t)n1);
      hc.put(&F.max_dist, in->max_dist1, (size_t)n1);
      if (do_search) hc.put(&P.mpdesc1, in->mp_desc1, (size_t)n1 * 32);
    }
    if (do_search) {
      hc.put(&P.obs1, in->mp_observed1, (size_t)n1);
      RGBL_TRY(put_features(hc, in->device2, n2, in->desc2, in->kp2_xy, in->kp2_octave, in->uright2, &P.desc2, &P.xy2, &P.oct2, &P.ur2));
      if (in->blocked2) hc.put(&P.blocked2, in->blocked2, (size_t)n2);
      F.valid1 = hc.scratch<uint8_t>(n1);
      F.proj1 = hc.scratch<float>((size_t)n1 * 3);
      F.level1 = hc.scratch<int32_t>(n1);
      F.viewcos1 = hc.scratch<float>(n1);
      if (pool) { F.mpdesc1 = hc.scratch<uint8_t>((size_t)n1 * 32); P.mpdesc1 = F.mpdesc1; }
      P.valid1 = F.valid1; P.proj1 = F.proj1; P.level1 = F.level1; P.viewcos1 = F.viewcos1;
    }
    F.in_view = hc.result<uint8_t>(n1);   // the results back to back: one copy back
    if (rec) F.rec = hc.result<rgbl_frustum_record>(n1);
    if (do_search) greedy_layout(hc, P);
    return RGBL_OK;
  }));
  memcpy(F.Rcw, in->Rcw, sizeof(F.Rcw));
  memcpy(F.tcw, in->tcw, sizeof(F.tcw));
  memcpy(F.Ow, in->Ow, sizeof(F.Ow));
  memcpy(F.K, in->K, sizeof(F.K));
  memcpy(F.bounds, in->grid, sizeof(F.bounds));
  F.mbf = in->mbf; F.log_scale = in->log_scale_factor; F.cos_limit = in->viewing_cos_limit;
  F.far_points = in->far_points; F.th_far = in->th_far_points; F.n_levels = in->n_levels;
  RGBL_TRY(launch(m, s, "k_frustum", k_frustum, dim3((n1 + 255) / 256), dim3(256), 0, F));
  if (do_search) {
    memcpy(P.grid, in->grid, sizeof(P.grid));
    P.th = in->th;
    P.nnratio = in->nnratio;
    set_scales(P, in->scale_factors, in->n_levels);
    RGBL_TRY(greedy_search(m, s, P, in->device2, {k_local_candidates, k_local_resolve<true>, k_local_resolve<false>, "k_local_candidates", "k_local_resolve"}));
  }
  RGBL_TRY(hc.fetch());
  memcpy(in_view, hc.host(F.in_view), (size_t)n1);
  if (rec) memcpy(rec, hc.host(F.rec), sizeof(rgbl_frustum_record) * (size_t)n1);
  int nv = 0;
  for (int i = 0; i < n1; ++i) nv += in_view[i] != 0;
  *n_in_view = nv;
  if (do_search) *out_nmatches = scatter_matches(hc.host(P.choice), n1, match2);
  return RGBL_OK;
}
}  // namespace

int rgbl_frustum_cull(rgbl_matcher* m, const rgbl_track_local_input* in, uint8_t* in_view, rgbl_frustum_record* rec, int* n_in_view) {
  return track_local_core(m, in, in_view, rec, n_in_view, false, nullptr, nullptr);
}

int rgbl_track_local_points(rgbl_matcher* m, const rgbl_track_local_input* in, uint8_t* in_view, rgbl_frustum_record* rec,
                            int* n_to_match, int32_t* match2, int* out_nmatches) {
  return track_local_core(m, in, in_view, rec, n_to_match, true, match2, out_nmatches);
}

// test hooks (tests/test_logf_glibc.py): the restatement on the host, and the same function compiled for the device
float rgbl_test_logf(float x) { return rgbl::logf_glibc(x); }
int rgbl_test_logf_device(const float* x, float* y, int n) {
  if (!x || !y || n < 1) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return elementwise_device_hook<float>({x}, y, n, [&](float* const* d, float* dy, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_test_logf, grid, block, 0, 0, (const float*)d[0], dy, n);
  });
}

int rgbl_search_for_initialization(rgbl_matcher* m, const rgbl_initialization_input* in, float* prev_matched, int32_t* matches12,
                                   int* out_nmatches) {
  if (!m || !in || !out_nmatches || in->n1 < 0 || in->n1 >= (1 << 20) || in->n2 < 0 || in->n2 > 65535 || (in->n1 > 0 && (!prev_matched || !matches12))) {
    set_error("invalid argument (the second frame may hold at most 65535 features, the first 2^20 - 1)");
    return RGBL_ERR_INVALID;
  }
  *out_nmatches = 0;
  const int n1 = in->n1, n2 = in->n2;
  for (int i = 0; i < n1; ++i) matches12[i] = -1;
  if (n1 == 0 || n2 == 0) return RGBL_OK;
  for (int i = 0; i < n1; ++i)
    if (in->kp1_octave[i] < 0) { set_error("negative octave"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  ProjDev P;
  memset(&P, 0, sizeof(P));
  P.n1 = n1; P.n2 = n2;
  RGBL_TRY(hc.begin([&]() -> int {
    hc.put(&P.proj1, (const float*)prev_matched, (size_t)n1 * 2);
    hc.put(&P.mpdesc1, in->desc1, (size_t)n1 * 32);
    hc.put(&P.oct1, in->kp1_octave, (size_t)n1);
    RGBL_TRY(put_features(hc, nullptr, n2, in->desc2, in->kp2_xy, in->kp2_octave, nullptr, &P.desc2, &P.xy2, &P.oct2, nullptr));
    P.owner = hc.result<int32_t>(n2);   // next to P.choice: one copy back
    greedy_layout(hc, P);
    return RGBL_OK;
  }));
  memcpy(P.grid, in->grid, sizeof(P.grid));
  P.th = (float)in->window_size;  // GetFeaturesInArea takes r as const float&
  P.nnratio = in->nnratio;
  // candidates at or above v cannot change a decision: as best they fail TH_LOW, as second-best they pass the ratio test
  // for every best <= TH_LOW
  int v = 51;
  while (v <= 256 && !((float)v * in->nnratio > 50.0f)) ++v;
  P.max_dist = v - 1;
  RGBL_TRY(greedy_search(m, s, P, nullptr, {k_init_candidates, k_init_resolve<true>, k_init_resolve<false>, "k_init_candidates", "k_init_resolve"}));
  RGBL_TRY(hc.fetch());
  const int32_t *choice = hc.host(P.choice), *owner = hc.host(P.owner);
  // a feature whose match was taken over later stays in the rotation histogram (pushed at match time, :720-730) but
  // holds no match any more (:708-712); nmatches always equals the number of entries >= 0
  RotationFilter rf;
  for (int i = 0; i < n1; ++i) {
    const int c = choice[i];
    if (c < 0) continue;
    if (owner[c] == i) matches12[i] = c;
    if (in->check_orientation) rf.add(i, in->kp1_angle[i], in->kp2_angle[c]);
  }
  if (in->check_orientation) rf.drop_outliers([&](int i) { matches12[i] = -1; });
  int nmatches = 0;
  for (int i = 0; i < n1; ++i)
    if (matches12[i] >= 0) {  // "Update prev matched" (:757-760)
      ++nmatches;
      prev_matched[2 * i] = in->kp2_xy[2 * matches12[i]];
      prev_matched[2 * i + 1] = in->kp2_xy[2 * matches12[i] + 1];
    }
  *out_nmatches = nmatches;
  return RGBL_OK;
}

// ---- vocabulary handle -----------------------------------------------------------------------------------------------
struct rgbl_vocabulary {
  int device = 0, k = 0, L = 0, n_nodes = 0, n_words = 0;
  VocDev dev{};
  std::vector<void*> allocs;
  hipStream_t stream = nullptr;
  // staging for the host entry point (grown on demand): ONE device block desc [cap x 32] | weight [cap] | word [cap] | node [cap]
  // and its page-locked mirror - one request up, one back
  uint8_t* d_stage = nullptr; uint8_t* h_stage = nullptr; int stage_cap = 0;
};

static int voc_upload(rgbl_vocabulary* v, int n_nodes, int L, const int32_t* child_off, const int32_t* child, const uint8_t* desc,
                      const double* weight, const int32_t* word_id) {
  auto up = [&](const void* src, size_t bytes, const void** dst) -> int {
    void* p = nullptr;
    RGBL_HIP(rgbl::device_alloc(&p, std::max<size_t>(bytes, 16)));
    v->allocs.push_back(p);
    RGBL_HIP(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = p;
    return RGBL_OK;
  };
  v->n_nodes = n_nodes; v->L = L;
  v->dev.n_nodes = n_nodes; v->dev.L = L;
  RGBL_TRY(up(child_off, sizeof(int32_t) * ((size_t)n_nodes + 1), (const void**)&v->dev.child_off));
  RGBL_TRY(up(child, sizeof(int32_t) * (size_t)std::max(n_nodes - 1, 1), (const void**)&v->dev.child));
  RGBL_TRY(up(desc, (size_t)n_nodes * 32, (const void**)&v->dev.desc));
  RGBL_TRY(up(weight, sizeof(double) * (size_t)n_nodes, (const void**)&v->dev.weight));
  RGBL_TRY(up(word_id, sizeof(int32_t) * (size_t)n_nodes, (const void**)&v->dev.word_id));
  RGBL_HIP(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
  return RGBL_OK;
}

static int voc_new(int device, rgbl_vocabulary** out) {
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device: librgbl_frontend has no CPU fallback"); return RGBL_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("device %d out of range", device); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(device));
  rgbl_vocabulary* v = new rgbl_vocabulary;
  v->device = device;
  *out = v;
  return RGBL_OK;
}

void rgbl_vocabulary_destroy(rgbl_vocabulary* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  for (void* p : v->allocs) (void)hipFree(p);
  if (v->d_stage) (void)hipFree(v->d_stage);
  if (v->h_stage) (void)hipHostFree(v->h_stage);
  if (v->stream) (void)hipStreamDestroy(v->stream);
  delete v;
}

int rgbl_vocabulary_create(int n_nodes, int L, const int32_t* child_off, const int32_t* child, const uint8_t* desc,
                           const double* weight, const int32_t* word_id, int device, rgbl_vocabulary** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (n_nodes < 2 || L < 1 || !child_off || !child || !desc || !weight || !word_id || child_off[0] != 0 ||
      child_off[n_nodes] != n_nodes - 1 || child_off[1] == 0) {
    set_error("vocabulary: the tree needs a root with children and n_nodes - 1 child entries");
    return RGBL_ERR_INVALID;
  }
  rgbl_vocabulary* v = nullptr;
  RGBL_TRY(voc_new(device, &v));
  int nw = 0, kmax = 0;
  for (int i = 0; i < n_nodes; ++i) {
    kmax = std::max(kmax, child_off[i + 1] - child_off[i]);
    nw += child_off[i + 1] == child_off[i];
  }
  v->k = kmax; v->n_words = nw;
  const int rc = voc_upload(v, n_nodes, L, child_off, child, desc, weight, word_id);
  if (rc != RGBL_OK) { rgbl_vocabulary_destroy(v); return rc; }
  *out = v;
  return RGBL_OK;
}

// ORBVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1425): "k L scoring weighting", then one node per line
// "parent is_leaf d0 .. d31 weight", node ids in file order starting at 1, word ids handed out to the leaves in file order.
// Only L1_NORM / TF_IDF files (ORBvoc.txt: "10 6 0 0") are accepted.  A trailing empty line is ignored here (the reference
// turns it into an extra child of the root with an unset descriptor).
int rgbl_vocabulary_load_text(const char* path, int device, rgbl_vocabulary** out) {
  if (!out || !path) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  FILE* f = fopen(path, "r");
  if (!f) { set_error("cannot open vocabulary file %s", path); return RGBL_ERR_INVALID; }
  int k = 0, L = 0, n1 = -1, n2 = -1;
  if (fscanf(f, "%d %d %d %d", &k, &L, &n1, &n2) != 4 || k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) {
    fclose(f);
    set_error("Vocabulary loading failure: This is not a correct text file!");
    return RGBL_ERR_INVALID;
  }
  if (n1 != 0 || n2 != 0) { fclose(f); set_error("only L1_NORM / TF_IDF vocabularies (scoring 0, weighting 0) are supported"); return RGBL_ERR_INVALID; }
  std::vector<int32_t> parent(1, 0), word(1, -1);
  std::vector<uint8_t> desc(32, 0), leaf(1, 0);
  std::vector<double> weight(1, 0.0);
  int nw = 0;
  for (;;) {
    int pid, is_leaf;
    if (fscanf(f, "%d %d", &pid, &is_leaf) != 2) break;
    const int nid = (int)parent.size();
    if (pid < 0 || pid >= nid) { fclose(f); set_error("vocabulary: node %d names parent %d", nid, pid); return RGBL_ERR_INVALID; }
    uint8_t d[32];
    for (int j = 0; j < 32; ++j) { int b; if (fscanf(f, "%d", &b) != 1) { fclose(f); set_error("vocabulary: truncated node %d", nid); return RGBL_ERR_INVALID; } d[j] = (uint8_t)b; }
    double w;
    if (fscanf(f, "%lf", &w) != 1) { fclose(f); set_error("vocabulary: truncated node %d", nid); return RGBL_ERR_INVALID; }
    parent.push_back(pid); leaf.push_back(is_leaf > 0); weight.push_back(w);
    desc.insert(desc.end(), d, d + 32);
    word.push_back(is_leaf > 0 ? nw++ : -1);
  }
  fclose(f);
  const int n = (int)parent.size();
  if (n < 2) { set_error("vocabulary: no nodes"); return RGBL_ERR_INVALID; }
  std::vector<int32_t> off(n + 1, 0), child(n - 1), fill(n, 0);
  for (int i = 1; i < n; ++i) ++off[parent[i] + 1];
  for (int i = 0; i < n; ++i) off[i + 1] += off[i];
  for (int i = 1; i < n; ++i) child[off[parent[i]] + fill[parent[i]]++] = i;
  for (int i = 1; i < n; ++i)
    if (leaf[i] && off[i + 1] != off[i]) { set_error("vocabulary: leaf %d has children", i); return RGBL_ERR_INVALID; }
  const int rc = rgbl_vocabulary_create(n, L, off.data(), child.data(), desc.data(), weight.data(), word.data(), device, out);
  if (rc == RGBL_OK) (*out)->k = k;
  return rc;
}

int rgbl_vocabulary_info(const rgbl_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words) {
  if (!v) { set_error("null handle"); return RGBL_ERR_INVALID; }
  if (k) *k = v->k;
  if (L) *L = v->L;
  if (n_nodes) *n_nodes = v->n_nodes;
  if (n_words) *n_words = v->n_words;
  return RGBL_OK;
}

int rgbl_bow_descend_batch_device(rgbl_vocabulary* v, void* hip_stream, const uint8_t* d_desc, const int32_t* d_n, int batch, int cap,
                                  int levelsup, int32_t* d_word, double* d_weight, int32_t* d_node) {
  if (!v || !d_desc || !d_word || !d_weight || !d_node || batch < 1 || cap < 1) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(v->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : v->stream;
  hipLaunchKernelGGL(k_bow_descend, dim3((cap + 255) / 256, batch), dim3(256), 0, s, v->dev, d_desc, d_n, cap, levelsup, d_word,
                     d_weight, d_node);
  RGBL_HIP(hipGetLastError());
  return RGBL_OK;
}

// void TemplatedVocabulary::transform(const std::vector<TDescriptor>& features, BowVector& v, FeatureVector& fv, int levelsup)
// (TemplatedVocabulary.h:1127-1192) for TF_IDF / L1_NORM: BowVector::addWeight in feature order, L1 normalisation summed in
// ascending word order, FeatureVector::addFeature with ascending feature indices; stopped words (weight 0) are dropped.
static int bow_transform_core(rgbl_vocabulary* v, const rgbl_device_frame* frame, const uint8_t* desc, int n, int levelsup,
                              uint32_t* word_id, double* word_val, int cap_words, int* n_words, uint32_t* node_id, int32_t* node_off,
                              uint32_t* node_feat, int cap_nodes, int* n_nodes) {
  if (!v || !n_words || !n_nodes || n < 0 || (n > 0 && !desc && !frame)) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  if (frame && frame->device != v->device) { set_error("device frame and vocabulary live on different devices"); return RGBL_ERR_INVALID; }
  *n_words = 0; *n_nodes = 0;
  if (n == 0) { if (node_off && cap_nodes >= 0) node_off[0] = 0; return RGBL_OK; }
  RGBL_HIP(hipSetDevice(v->device));
  if (n > v->stage_cap) {
    if (v->d_stage) { (void)hipFree(v->d_stage); (void)hipHostFree(v->h_stage); }
    v->d_stage = nullptr; v->h_stage = nullptr; v->stage_cap = 0;
    const int cap = std::max(n, 4096);
    RGBL_HIP(rgbl::device_alloc(&v->d_stage, (size_t)cap * 48));
    RGBL_HIP(rgbl::pinned_alloc(&v->h_stage, (size_t)cap * 48));
    v->stage_cap = cap;
  }
  RGBL_HIP(refill_staging(v->d_stage, v->h_stage, (size_t)v->stage_cap * 48, v->stream));
  const size_t cap = (size_t)v->stage_cap;   // results back to back: weight [n] | word [n] | node [n]
  const uint8_t* d_desc = v->d_stage;
  double* d_weight = reinterpret_cast<double*>(v->d_stage + cap * 32);
  int32_t* d_word = reinterpret_cast<int32_t*>(d_weight + n);
  int32_t* d_node = d_word + n;
  hipStream_t s = v->stream;
  StreamDrain drain(s);  // error returns included
  if (frame) {   // the frame's descriptors are resident: nothing goes up
    RGBL_HIP(hipStreamWaitEvent(s, frame->ready, 0));
    d_desc = frame->d_desc;
  } else {
    memcpy(v->h_stage, desc, (size_t)n * 32);
    RGBL_HIP(hipMemcpyAsync(v->d_stage, v->h_stage, (size_t)n * 32, hipMemcpyHostToDevice, s));
  }
  hipLaunchKernelGGL(k_bow_descend, dim3((n + 255) / 256, 1), dim3(256), 0, s, v->dev, d_desc, (const int32_t*)nullptr, n, levelsup,
                     d_word, d_weight, d_node);
  RGBL_HIP(hipGetLastError());
  RGBL_HIP(hipMemcpyAsync(v->h_stage + cap * 32, v->d_stage + cap * 32, (size_t)n * 16, hipMemcpyDeviceToHost, s));
  RGBL_HIP(hipStreamSynchronize(s));
  const double* weight = reinterpret_cast<const double*>(v->h_stage + cap * 32);
  const int32_t* word = reinterpret_cast<const int32_t*>(weight + n);
  const int32_t* node = word + n;
  // the two std::map containers of the reference, as sorted (key << 32 | feature) runs: one unstable sort of 64-bit integers each
  // (the feature index makes the keys distinct, so the order inside a word / node is the order of the features) on buffers the
  // thread keeps - round 6: 2 x stable_sort of pairs in freshly grown vectors was ~25 us of a 72-us call
  static thread_local std::vector<unsigned long long> wf, nf;
  wf.clear(); nf.clear();
  for (int i = 0; i < n; ++i)
    if (weight[i] > 0) {
      wf.push_back(((unsigned long long)(uint32_t)word[i] << 32) | (uint32_t)i);
      nf.push_back(((unsigned long long)(uint32_t)node[i] << 32) | (uint32_t)i);
    }
  std::sort(wf.begin(), wf.end());
  std::sort(nf.begin(), nf.end());
  int nw = 0, nn = 0;
  for (size_t a = 0; a < wf.size();) {
    size_t b = a;
    double acc = 0.0;
    bool first = true;
    for (; b < wf.size() && (wf[b] >> 32) == (wf[a] >> 32); ++b) {
      const double w = weight[(uint32_t)wf[b]];
      acc = first ? w : acc + w;
      first = false;
    }
    if (nw < cap_words && word_id && word_val) { word_id[nw] = (uint32_t)(wf[a] >> 32); word_val[nw] = acc; }
    ++nw;
    a = b;
  }
  for (size_t a = 0; a < nf.size();) {
    size_t b = a;
    while (b < nf.size() && (nf[b] >> 32) == (nf[a] >> 32)) ++b;
    if (nn < cap_nodes && node_id && node_off && node_feat) {
      node_id[nn] = (uint32_t)(nf[a] >> 32);
      node_off[nn] = (int32_t)a;
      for (size_t q = a; q < b; ++q) node_feat[q] = (uint32_t)nf[q];
    }
    ++nn;
    a = b;
  }
  *n_words = nw; *n_nodes = nn;
  if (nw > cap_words || nn > cap_nodes) { set_error("BoW transform: %d words / %d nodes exceed the output capacity", nw, nn); return RGBL_ERR_CAPACITY; }
  if (node_off) node_off[nn] = (int32_t)nf.size();
  double norm = 0.0;  // BowVector::normalize(L1)
  for (int i = 0; i < nw; ++i) norm += fabs(word_val[i]);
  if (norm > 0.0)
    for (int i = 0; i < nw; ++i) word_val[i] /= norm;
  return RGBL_OK;
}

int rgbl_bow_transform(rgbl_vocabulary* v, const uint8_t* desc, int n, int levelsup, uint32_t* word_id, double* word_val,
                       int cap_words, int* n_words, uint32_t* node_id, int32_t* node_off, uint32_t* node_feat, int cap_nodes,
                       int* n_nodes) {
  return bow_transform_core(v, nullptr, desc, n, levelsup, word_id, word_val, cap_words, n_words, node_id, node_off, node_feat, cap_nodes,
                            n_nodes);
}

int rgbl_bow_transform_frame(rgbl_vocabulary* v, const rgbl_device_frame* frame, int levelsup, uint32_t* word_id, double* word_val,
                             int cap_words, int* n_words, uint32_t* node_id, int32_t* node_off, uint32_t* node_feat, int cap_nodes,
                             int* n_nodes) {
  if (!frame) { set_error("null frame"); return RGBL_ERR_INVALID; }
  return bow_transform_core(v, frame, nullptr, frame->n, levelsup, word_id, word_val, cap_words, n_words, node_id, node_off, node_feat,
                            cap_nodes, n_nodes);
}

// device part of both SearchByBoW overloads over the shared nodes `sn` of (kf, fr): match1[idx1] = feature of `fr` taken by
// key-frame feature idx1 (or -1), match2 the inverse; a caller passes nullptr for the one it does not want, and has filled the
// other with -1
// a second-set feature's bucket position indexes BowLds::taken (and travels in the low 16 bits of the search key): the entry points
// refuse a larger bucket before they write anything
static int check_bow_buckets(const SharedNodes& sn) {
  const rgbl_keyframe_view* fr = sn.b;
  if (sn.empty()) return RGBL_OK;
  for (int p = 0; p < sn.npairs(); ++p)
    if (fr->node_off[sn.pb[p] + 1] - fr->node_off[sn.pb[p]] > kBowBucket) {
      set_error("SearchByBoW: a vocabulary node holds more than %d features of the second set", kBowBucket);
      return RGBL_ERR_INVALID;
    }
  return RGBL_OK;
}

static int bow_core(rgbl_matcher* m, const SharedNodes& sn, float nnratio, bool second_needs_mp, int max_best, int n_left2,
                    int32_t* match1, int32_t* match2) {
  const rgbl_keyframe_view *kf = sn.a, *fr = sn.b;
  const int n1 = kf->n, n2 = fr->n, npairs = sn.npairs();
  if (sn.empty()) return RGBL_OK;
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // error returns included
  HostCall hc(m);
  hipStream_t s = hc.s;
  BowDev T;
  T.valid2 = nullptr;
  RGBL_TRY(hc.begin([&]() -> int {
    RGBL_TRY(sn.put(hc, {&T.desc1}, {&T.desc2}, T.fv));
    hc.put(&T.valid1, kf->has_mappoint, (size_t)n1);
    if (second_needs_mp) hc.put(&T.valid2, fr->has_mappoint, (size_t)n2);
    T.match1 = hc.put_fill<int32_t>(n1, 0xff);   // all -1: travel with the upload
    T.match2 = hc.put_fill<int32_t>(n2, 0xff);
    hc.mark_result(T.match1, n1);
    hc.mark_result(T.match2, n2);
    return RGBL_OK;
  }));
  T.nnratio = nnratio;
  T.max_best = max_best;
  T.n_left2 = n_left2;
  if (n_left2 >= 0) RGBL_TRY(launch(m, s, "k_search_by_bow_rig", k_search_by_bow_rig, dim3(npairs), dim3(64), 0, T));
  else RGBL_TRY(launch(m, s, "k_search_by_bow", k_search_by_bow, dim3(npairs), dim3(64), 0, T));
  RGBL_TRY(hc.fetch());
  if (match1) memcpy(match1, hc.host(T.match1), sizeof(int32_t) * n1);
  if (match2) memcpy(match2, hc.host(T.match2), sizeof(int32_t) * n2);
  return RGBL_OK;
}

int rgbl_search_by_bow(rgbl_matcher* m, const rgbl_keyframe_view* kf, const rgbl_keyframe_view* fr, float nnratio,
                       int check_orientation, int32_t* match_f, int* out_nmatches) {
  return rgbl_search_by_bow_rig(m, kf, fr, -1, nnratio, check_orientation, match_f, out_nmatches);
}

// The same with F.Nleft (-1: a single camera): a key-frame feature may hand its map point to a left AND a right frame feature
// (ORBmatcher.cc:298-326, 357-386), so the rotation histogram is filled from the frame's side - its bins' SIZES are all that
// ComputeThreeMaxima reads (:403-421), and every matched frame feature is in exactly one bin.
int rgbl_search_by_bow_rig(rgbl_matcher* m, const rgbl_keyframe_view* kf, const rgbl_keyframe_view* fr, int frame_n_left, float nnratio,
                           int check_orientation, int32_t* match_f, int* out_nmatches) {
  if (!m || !kf || !fr || !match_f || !out_nmatches || kf->n < 0 || fr->n < 0 || frame_n_left < -1 || frame_n_left > fr->n) {
    set_error("invalid argument");
    return RGBL_ERR_INVALID;
  }
  const SharedNodes sn(kf, fr);
  RGBL_TRY(check_bow_buckets(sn));
  *out_nmatches = 0;
  const int n2 = fr->n;
  for (int i = 0; i < n2; ++i) match_f[i] = -1;
  RGBL_TRY(bow_core(m, sn, nnratio, false, 50 /* <= TH_LOW */, frame_n_left, nullptr, match_f));
  int nmatches = 0;
  for (int i = 0; i < n2; ++i) nmatches += match_f[i] >= 0;
  if (check_orientation) {
    RotationFilter rf;
    for (int idx2 = 0; idx2 < n2; ++idx2)
      if (match_f[idx2] >= 0) rf.add(idx2, kf->kp_angle[match_f[idx2]], fr->kp_angle[idx2]);
    rf.drop_outliers([&](int idx2) { match_f[idx2] = -1; --nmatches; });
  }
  *out_nmatches = nmatches;
  return RGBL_OK;
}

// int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBmatcher.cc:765-905):
// both sides need a good map point, the best distance must be < TH_LOW, the result is indexed by the first key frame.
int rgbl_search_by_bow_keyframes(rgbl_matcher* m, const rgbl_keyframe_view* kf1, const rgbl_keyframe_view* kf2, float nnratio,
                                 int check_orientation, int32_t* match12, int* out_nmatches) {
  if (!m || !kf1 || !kf2 || !match12 || !out_nmatches || kf1->n < 0 || kf2->n < 0) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const SharedNodes sn(kf1, kf2);
  RGBL_TRY(check_bow_buckets(sn));
  *out_nmatches = 0;
  for (int i = 0; i < kf1->n; ++i) match12[i] = -1;
  RGBL_TRY(bow_core(m, sn, nnratio, true, 49 /* < TH_LOW */, -1, match12, nullptr));
  finish_matches12(sn, match12, check_orientation != 0, out_nmatches);
  return RGBL_OK;
}

}  // extern "C"
