// gba.hip — Optimizer::BundleAdjustment (src/Optimizer.cc:52-390), the global bundle adjustment, as ONE problem spread over
// the device.  The edges, the Schur complement and Levenberg's control are csrc/lba_math.h's and the per-item kernels are
// lba.hip's (csrc/lba_call.h has the scaffold both calls share); what is new here is the reduced camera system: up to 1 024
// active cameras, n = 6 144 unknowns, where LocalBundleAdjustment's one-workgroup k_lba_factor is out of the question.
// lm_solve_panel of csrc/lm_math.h is the host text; the kernels below run its loops with an element or a row per work-item.
// Every dependency is a kernel boundary: no grid-wide barrier, no cooperative launch, no spin-wait, no atomics, no captured
// graph; fp64 VALU arithmetic without contraction and without the matrix instructions (a fused accumulate would leave the
// host's bits).
//
//   per trial          k_gba_schur      one workgroup per upper block of S that is NOT empty (every diagonal block, the others
//                                       with a pair of edges); S is zeroed before, so an empty block reads as k_lba_schur leaves it
//   per panel of W     k_gba_diag       (b) one workgroup: the W x W diagonal block through the panel's own columns, the pivots
//   columns            k_gba_rows       (c) one row below the panel per work-item, the block's L and D in LDS
//                      k_gba_trailing   (a) 64 x 64 tiles of everything behind the panel: each element continues its sum through
//                                       the panel's W columns, 16 elements per work-item in registers, the L_i., L_j. and D
//                                       slices in LDS - so every column has been through all p before its panel when its turn comes
//   forward, per panel k_gba_forward    the block's triangle (recomputed per workgroup from values no launch of this kernel
//                                       writes), then the finished block on every row below
//                      k_gba_scale      y / D
//   backward, per      k_gba_backward   the mirror: the block's triangle from the last column up, then the finished block on
//   panel, last first                   every row above - p descending per element
//                      k_gba_finish     the cameras' trial estimates and the record's ok
// A failed pivot sets V.pfail in k_gba_diag; every later kernel of the solve reads it first and leaves (uniformly, before any
// barrier), so x_cam keeps what it held and k_gba_finish reports ok = 0.  Every loop is bounded by n or W.
#include <string.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "matcher_call.h"
#include "lba_math.h"
#include "lba_call.h"

namespace rgbl {

constexpr int kGbaMaxCams = 2048;      // cameras a call may list
constexpr int kGbaMaxActive = 1024;    // active ones: the reduced system is dense, 6 144^2 / 2 doubles = 151 MB
constexpr int kGbaTile = 64;           // rows and columns of one k_gba_trailing tile
constexpr int kGbaRowBlock = 64;       // work-items of k_gba_rows
constexpr int kGbaVecBlock = 256;      // work-items of the substitution kernels

__global__ __launch_bounds__(kLbaSchurLanes) void k_gba_schur(LbaView V, double lambda) {
  const int b = (int)blockIdx.x;
  lba_schur_lane(V, lambda, V.blk_list[2 * (size_t)b], V.blk_list[2 * (size_t)b + 1], (int)threadIdx.x);
}

// (a) behind a finished panel [j0, j0 + W): every element (i, j) of the columns j >= j0 + W continues its sum through the
// panel's W columns and goes back to S - so a panel's own columns have been through every p before it when its turn comes,
// p ascending, one subtraction at a time, exactly lm_solve_panel's (a).  (Carrying an element through ALL earlier columns in
// one launch, as the host text's loop does, has only the n W elements of one panel to spread: at W = 32 fewer than a fifth of
// the device's compute units get a tile; measured in DESIGN.md 9.)  One 64 x 64 tile of the lower triangle per workgroup,
// grid (tile column, tile row): tiles above the diagonal leave at once.  Work-item (ty, tx) owns rows ty + 16 a and columns
// tx + 16 b, a, b = 0 .. 3.
template <int W> __global__ __launch_bounds__(256) void k_gba_trailing(LbaView V, int j0) {
  __shared__ double s_li[kGbaTile][W + 1], s_lj[W][kGbaTile], s_d[W];
  if (blockIdx.x > blockIdx.y || *V.pfail) return;
  const int n = V.n, tid = (int)threadIdx.x, ty = tid / 16, tx = tid % 16;
  const int i0 = j0 + W + (int)blockIdx.y * kGbaTile, c0 = j0 + W + (int)blockIdx.x * kGbaTile;
  for (int t = tid; t < kGbaTile * W; t += 256) {
    const int p = t % W, r = t / W;
    s_li[r][p] = i0 + r < n ? V.S[lm_tri((size_t)(i0 + r), (size_t)(j0 + p))] : 0.0;
    s_lj[p][r] = c0 + r < n ? V.S[lm_tri((size_t)(c0 + r), (size_t)(j0 + p))] : 0.0;
  }
  if (tid < W) s_d[tid] = V.pD[j0 + tid];
  __syncthreads();
  double v[4][4];
  bool mine[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = c0 + tx + 16 * b;
      mine[a][b] = i < n && j <= i;
      v[a][b] = mine[a][b] ? V.S[lm_tri((size_t)i, (size_t)j)] : 0.0;
    }
#pragma unroll 4
  for (int p = 0; p < W; ++p) {
    const double d = s_d[p];
    double li[4], lj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { li[a] = s_li[ty + 16 * a][p]; lj[a] = s_lj[p][tx + 16 * a]; }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) v[a][b] = v[a][b] - li[a] * lj[b] * d;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (mine[a][b]) V.S[lm_tri((size_t)(i0 + ty + 16 * a), (size_t)(c0 + tx + 16 * b))] = v[a][b];
}

// (b) the diagonal block: column by column, row i of the block on work-item i
template <int W> __global__ __launch_bounds__(64) void k_gba_diag(LbaView V, int j0) {
  static_assert(W <= 64, "one work-item per row of the block");
  __shared__ double s_b[W][W + 1], s_d[W];
  if (*V.pfail) return;
  const int n = V.n, i = (int)threadIdx.x, wn = n - j0 < W ? n - j0 : W;
  if (i < wn)
    for (int c = 0; c <= i; ++c) s_b[i][c] = V.S[lm_tri((size_t)(j0 + i), (size_t)(j0 + c))];
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < wn && ok; ++j) {
    if (i >= j && i < wn) {
      double v = s_b[i][j];
      for (int p = 0; p < j; ++p) v = v - s_b[i][p] * s_b[j][p] * s_d[p];
      s_b[i][j] = v;
    }
    __syncthreads();
    const double d = s_b[j][j];
    ok = d > 0.0 && d <= DBL_MAX;
    if (ok) {
      if (i == j) s_d[j] = d;
      if (i > j && i < wn) s_b[i][j] = s_b[i][j] / d;
    }
    __syncthreads();
  }
  if (ok && i < wn) {
    for (int c = 0; c <= i; ++c) V.S[lm_tri((size_t)(j0 + i), (size_t)(j0 + c))] = s_b[i][c];
    V.pD[j0 + i] = s_d[i];
  }
  if (i == 0) *V.pfail = ok ? 0 : 1;   // only reached while no earlier panel failed
}

// (c) row i below the panel: its W entries in registers, each through the panel's own columns and divided by the pivot
template <int W> __global__ __launch_bounds__(kGbaRowBlock) void k_gba_rows(LbaView V, int j0) {
  __shared__ double s_l[W][W], s_d[W];
  if (*V.pfail) return;
  const int n = V.n, tid = (int)threadIdx.x;
  for (int t = tid; t < W * W; t += kGbaRowBlock) {
    const int c = t / W, p = t % W;
    s_l[c][p] = p < c ? V.S[lm_tri((size_t)(j0 + c), (size_t)(j0 + p))] : 0.0;
  }
  for (int t = tid; t < W; t += kGbaRowBlock) s_d[t] = V.pD[j0 + t];
  __syncthreads();
  const int i = j0 + W + (int)(blockIdx.x * kGbaRowBlock) + tid;
  if (i >= n) return;
  double* row = V.S + lm_tri((size_t)i, (size_t)j0);
  double l[W];
#pragma unroll
  for (int c = 0; c < W; ++c) l[c] = row[c];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    double v = l[c];
#pragma unroll
    for (int p = 0; p < c; ++p) v = v - l[p] * s_l[c][p] * s_d[p];
    l[c] = v / s_d[c];
  }
#pragma unroll
  for (int c = 0; c < W; ++c) row[c] = l[c];
}

__global__ __launch_bounds__(kGbaVecBlock) void k_gba_start(LbaView V) {
  if (*V.pfail) return;
  const int i = (int)(blockIdx.x * kGbaVecBlock + threadIdx.x);
  if (i < V.n) V.py[i] = V.bs[i];
}
// The block's triangle in LDS - its inputs py[j0 .. j1) are final and no workgroup of this launch writes them; workgroup 0
// keeps the result in pyf - then row i >= j1 subtracts L_ip y_p over the block, p ascending.
template <int W> __global__ __launch_bounds__(kGbaVecBlock) void k_gba_forward(LbaView V, int j0) {
  __shared__ double s_y[W];
  if (*V.pfail) return;
  const int n = V.n, tid = (int)threadIdx.x, wn = n - j0 < W ? n - j0 : W;
  if (tid < wn) s_y[tid] = V.py[j0 + tid];
  for (int p = 0; p + 1 < wn; ++p) {
    __syncthreads();
    if (tid > p && tid < wn) s_y[tid] = s_y[tid] - V.S[lm_tri((size_t)(j0 + tid), (size_t)(j0 + p))] * s_y[p];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < wn) V.pyf[j0 + tid] = s_y[tid];
  const int i = j0 + W + (int)(blockIdx.x * kGbaVecBlock) + tid;
  if (i >= n) return;
  const double* row = V.S + lm_tri((size_t)i, (size_t)j0);
  double v = V.py[i];
  for (int p = 0; p < W; ++p) v = v - row[p] * s_y[p];
  V.py[i] = v;
}
__global__ __launch_bounds__(kGbaVecBlock) void k_gba_scale(LbaView V) {
  if (*V.pfail) return;
  const int i = (int)(blockIdx.x * kGbaVecBlock + threadIdx.x);
  if (i < V.n) V.pxw[i] = V.pyf[i] / V.pD[i];
}
// The mirror: the block's x from its last column up (pxw[j0 .. j1) is final, and only read here), kept in x_cam by
// workgroup 0; then row i < j0 subtracts L_pi x_p over the block, p descending.
template <int W> __global__ __launch_bounds__(kGbaVecBlock) void k_gba_backward(LbaView V, int j0) {
  __shared__ double s_x[W];
  if (*V.pfail) return;
  const int n = V.n, tid = (int)threadIdx.x, wn = n - j0 < W ? n - j0 : W;
  if (tid < wn) s_x[tid] = V.pxw[j0 + tid];
  for (int p = wn - 1; p >= 1; --p) {
    __syncthreads();
    if (tid < p) s_x[tid] = s_x[tid] - V.S[lm_tri((size_t)(j0 + p), (size_t)(j0 + tid))] * s_x[p];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < wn) V.x_cam[j0 + tid] = s_x[tid];
  const int i = (int)(blockIdx.x * kGbaVecBlock) + tid;
  if (i >= j0) return;
  double v = V.pxw[i];
  for (int p = wn - 1; p >= 0; --p) v = v - V.S[lm_tri((size_t)(j0 + p), (size_t)i)] * s_x[p];
  V.pxw[i] = v;
}
// the trial estimate of every active camera - after a failed factorisation from the x the cameras hold - and the record's ok
__global__ __launch_bounds__(kLbaBlock) void k_gba_finish(LbaView V) {
  const int a = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (a < V.nA) lba_trial_camera(V, a);
  if (a == 0) V.rec->ok = (V.n > 0 && *V.pfail) ? 0 : 1;
}

}  // namespace rgbl

using namespace rgbl;
using namespace rgbl_lba;

namespace {
unsigned ceil_div(int items, int per) { return (unsigned)((items + per - 1) / per); }

// the reduced system of one trial: S over the blocks that are not empty, then lm_solve_panel's schedule, W columns per panel
template <int W> void gba_reduced(LbaDeviceBackend& B, double lambda) {
  const LbaView& V = B.V;
  const int n = V.n;
  if (n == 0) {
    B.launch("k_gba_finish", k_gba_finish, dim3(1), dim3(kLbaBlock), V);
    return;
  }
  if (B.rc == RGBL_OK) {
    hipError_t e = hipMemsetAsync(V.S, 0, sizeof(double) * lm_tri((size_t)n, 0), B.s);
    if (e == hipSuccess) e = hipMemsetAsync(V.pfail, 0, sizeof(int32_t), B.s);
    if (e != hipSuccess) { set_error("BA: %s", hipGetErrorString(e)); B.rc = RGBL_ERR_HIP; }
  }
  B.launch("k_gba_schur", k_gba_schur, dim3((unsigned)V.n_blk_list), dim3(kLbaSchurLanes), V, lambda);
  for (int j0 = 0; j0 < n; j0 += W) {
    B.launch("k_gba_diag", k_gba_diag<W>, dim3(1), dim3(64), V, j0);
    if (j0 + W >= n) break;
    const unsigned tiles = ceil_div(n - j0 - W, kGbaTile);
    B.launch("k_gba_rows", k_gba_rows<W>, dim3(ceil_div(n - j0 - W, kGbaRowBlock)), dim3(kGbaRowBlock), V, j0);
    B.launch("k_gba_trailing", k_gba_trailing<W>, dim3(tiles, tiles), dim3(256), V, j0);
  }
  B.launch("k_gba_start", k_gba_start, dim3(ceil_div(n, kGbaVecBlock)), dim3(kGbaVecBlock), V);
  for (int j0 = 0; j0 < n; j0 += W)
    B.launch("k_gba_forward", k_gba_forward<W>, dim3(std::max(1u, ceil_div(n - j0 - W, kGbaVecBlock))), dim3(kGbaVecBlock), V, j0);
  B.launch("k_gba_scale", k_gba_scale, dim3(ceil_div(n, kGbaVecBlock)), dim3(kGbaVecBlock), V);
  for (int j0 = (n - 1) / W * W; j0 >= 0; j0 -= W)
    B.launch("k_gba_backward", k_gba_backward<W>, dim3(std::max(1u, ceil_div(j0, kGbaVecBlock))), dim3(kGbaVecBlock), V, j0);
  B.launch("k_gba_finish", k_gba_finish, dim3(ceil_div(V.nA, kLbaBlock)), dim3(kLbaBlock), V);
}

// the call as LocalBundleAdjustment's scaffold reads it: every camera in the free list, the fixed flag per camera
rgbl_lba_input as_lba_input(const rgbl_ba_input* in) {
  rgbl_lba_input I;
  memset(&I, 0, sizeof(I));
  I.n_free = in->n_cams; I.n_fixed = 0; I.free_is_fixed = in->cam_is_fixed;
  I.cam_q = in->cam_q; I.cam_t = in->cam_t; I.cam_K = in->cam_K; I.cam_bf = in->cam_bf;
  I.n_points = in->n_points; I.world_pos = in->world_pos; I.pool = in->pool; I.slot = in->slot;
  I.n_edges = in->n_edges; I.edge_point = in->edge_point; I.edge_cam = in->edge_cam; I.edge_obs = in->edge_obs;
  I.edge_inv_sigma2 = in->edge_inv_sigma2;
  I.max_iterations = in->max_iterations; I.user_lambda_init = 0.0;
  I.stop = in->stop; I.stop_after_polls = in->stop_after_polls; I.stop_byte = in->stop_byte;
  return I;
}
int check_ba_input(const rgbl_ba_input* in, const rgbl_lba_input& I, bool host_only, LbaProblem& P) {
  P.what = "BA"; P.max_listed = kGbaMaxCams; P.max_active = kGbaMaxActive; P.panel = true;
  if (in->robust != 0 && in->robust != 1) { set_error("BA: robust is 0 or 1"); return RGBL_ERR_INVALID; }
  P.robust = in->robust != 0;
  P.delta[0] = (double)(float)sqrt(5.99); P.delta[1] = (double)(float)sqrt(7.815);   // thHuber2D, thHuber3D (:131-132): 5.99, not 5.991
  return check_lba_input(&I, host_only, P);
}
void write_ba_output(const rgbl_lba_input& I, rgbl_ba_output* out, const LbaProblem& P, const PoPose* T, const double* X,
                     const double* chi2, const LbaCounters& D, const LbaStop& stop) {
  rgbl_lba_output O;
  memset(&O, 0, sizeof(O));
  O.cam_q = out->cam_q; O.cam_t = out->cam_t; O.point = out->point; O.chi2 = out->chi2;
  O.diag.cam_q = out->diag.cam_q; O.diag.cam_t = out->diag.cam_t; O.diag.point = out->diag.point;
  write_lba_output(&I, &O, P, T, X, chi2, nullptr, D, stop);
  out->diag = O.diag;
  if (out->included)
    for (int p = 0; p < P.nP; ++p) out->included[p] = P.pt_off[(size_t)p + 1] > P.pt_off[(size_t)p] ? 1 : 0;   // :266-270
}
}  // namespace

int rgbl_bundle_adjustment_host(const rgbl_ba_input* in, rgbl_ba_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  const rgbl_lba_input I = as_lba_input(in);
  LbaProblem P;
  RGBL_TRY(check_ba_input(in, I, true, P));
  RGBL_TRY(build_lba_structure(&I, P));
  LbaStop stop = {in->stop, in->stop_byte, in->stop_after_polls, 0};
  P.X.resize(3 * (size_t)P.nP);
  for (size_t i = 0; i < P.X.size(); ++i) P.X[i] = (double)in->world_pos[i];   // :149
  const LbaOffsets O = lba_offsets(P);
  std::vector<uint8_t> mem(O.total, 0);
  lba_fill(&I, P, O, [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(mem.data() + off, src, bytes); });
  LbaHostBackend B;
  B.V = lba_view(P, O, mem.data());
  B.panel = true;
  B.D.resize((size_t)B.V.n); B.y.resize((size_t)B.V.n);
  LbaCounters D;
  lm_levenberg_loop(B, P.nE > 0 ? in->max_iterations : 0, 0.0, stop, D);
  write_ba_output(I, out, P, B.V.T, B.V.X, B.V.e_chi2, D, stop);
  return RGBL_OK;
}

int rgbl_bundle_adjustment(rgbl_matcher* m, const rgbl_ba_input* in, rgbl_ba_output* out) {
  if (!m || !in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  const rgbl_lba_input I = as_lba_input(in);
  LbaProblem P;
  RGBL_TRY(check_ba_input(in, I, false, P));
  PoolCall pc(m, "BA", "a frame");
  RGBL_TRY(pc.note(in->pool, {}, -1));
  RGBL_TRY(pc.lock(1, [&](int) -> int { return check_lba_slots(pc, in->slot, P); }));
  float* d_wpos = pc.pool ? pc.pool->d_wpos : nullptr;
  RGBL_TRY(build_lba_structure(&I, P));
  LbaStop stop = {in->stop, in->stop_byte, in->stop_after_polls, 0};
  if (!in->pool) {
    P.X.resize(3 * (size_t)P.nP);
    for (size_t i = 0; i < P.X.size(); ++i) P.X[i] = (double)in->world_pos[i];   // :149
  }
  const LbaOffsets O = lba_offsets(P);
  // the page-locked side: the record, then what comes back (T | X | e_chi2)
  const size_t back_begin = O.T, back_end = O.e_chi2 + sizeof(double) * (size_t)P.nE, pin_back = 256;
  RGBL_HIP(hipSetDevice(m->device));
  RGBL_TRY(ensure_arena(m, O.total));   // a device that cannot hold the call: RGBL_ERR_HIP, nothing launched or written
  RGBL_TRY(ensure_pin(m, pin_back + (back_end - back_begin)));
  LbaDeviceBackend B;
  B.m = m; B.s = m->stream; B.what = "BA";
  B.reduced = m->gba_panel == 16 ? gba_reduced<16> : m->gba_panel == 64 ? gba_reduced<64> : gba_reduced<kLmPanel>;
  uint8_t *d_buf = m->d_buf, *h_pin = m->h_pin;
  StreamDrain drain(B.s);   // behind pc (PoolCall): the stream is idle before the pool is released
  B.V = lba_view(P, O, d_buf);
  B.h_rec = reinterpret_cast<LbaRecord*>(h_pin);
  RGBL_HIP(hipMemsetAsync(d_buf, 0, O.total, B.s));
  int rc = RGBL_OK;
  lba_fill(&I, P, O, [&](size_t off, const void* src, size_t bytes) {
    if (!bytes || rc != RGBL_OK) return;
    const hipError_t e = hipMemcpyAsync(d_buf + off, src, bytes, hipMemcpyHostToDevice, B.s);   // pageable sources: staged by the runtime before it returns
    if (e != hipSuccess) { set_error("BA: upload: %s", hipGetErrorString(e)); rc = RGBL_ERR_HIP; }
  });
  RGBL_TRY(rc);
  const int32_t* d_slot = reinterpret_cast<const int32_t*>(d_buf + O.slot);
  if (in->pool && P.nP > 0) B.launch("k_lba_gather_points", k_lba_gather_points, dim3(B.blocks(P.nP)), dim3(kLbaBlock), B.V, (const float*)d_wpos, d_slot);
  LbaCounters D;
  const bool done = lm_levenberg_loop(B, P.nE > 0 ? in->max_iterations : 0, 0.0, stop, D);
  if (!done) return B.rc;
  if (in->pool && P.nP > 0) B.launch("k_lba_pool_write", k_lba_pool_write, dim3(B.blocks(P.nP)), dim3(kLbaBlock), B.V, d_wpos, d_slot);
  RGBL_TRY(B.rc);
  RGBL_HIP(hipMemcpyAsync(h_pin + pin_back, d_buf + back_begin, back_end - back_begin, hipMemcpyDeviceToHost, B.s));
  RGBL_HIP(hipStreamSynchronize(B.s));
  m->timer.collect();
  const uint8_t* back = h_pin + pin_back - back_begin;
  write_ba_output(I, out, P, reinterpret_cast<const PoPose*>(back + O.T), reinterpret_cast<const double*>(back + O.X),
                  reinterpret_cast<const double*>(back + O.e_chi2), D, stop);
  return RGBL_OK;
}
