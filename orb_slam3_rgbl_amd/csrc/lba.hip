// lba.hip — Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1188-1497) as ONE problem spread over the device.  The
// arithmetic, every summation order and Levenberg's scalar control are csrc/lba_math.h's; a kernel here hands each work-item the
// item it owns, the host build (rgbl_local_bundle_adjustment_host) runs the same functions in loops.  Every dependency is a
// kernel boundary: no grid-wide barrier, no cooperative launch, no spin-wait, no atomics, no captured graph.  The Levenberg
// loop runs on the host between launches and reads back one LbaRecord per pass (the stop flag lives in host memory and is
// polled where g2o polls it; every loop on the device stays bounded).
//
//   per iteration   k_lba_linearise     one edge per work-item: error, Jacobians, Huber, the edge's blocks
//                   k_lba_point_sums    one point per work-item: Hll_p, b_p over its edges
//                   k_lba_cam_blocks    one wave per active camera: Hpp_c, b_c, 64 lanes and the fixed tree
//                   k_lba_sums          one workgroup: the robust chi2 and computeLambdaInit's maximum
//   per trial       k_lba_trial_edges   one edge per work-item: B Dinv and B (Dinv b_p) at the trial's lambda
//                   k_lba_schur         one workgroup per upper block (i, j) of the reduced system, walking its pair list
//                   k_lba_factor        ONE workgroup: LDL^T and the solve (the triangle in LDS up to n = 120, in global memory
//                                       beyond), then the cameras' trial estimates
//                   k_lba_trial_points  one point per work-item: back-substitution, the trial estimate, its edges' chi2
//                   k_lba_sums          the trial's robust chi2 and computeScale
//   at the end      k_lba_flags         one edge per work-item; k_lba_pool_write with a pool
#include <string.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "matcher_call.h"
#include "lba_math.h"
#include "lba_call.h"   // the problem, its checks and lists, the layout and the two executions of the passes: shared with gba.hip

namespace rgbl {

__global__ __launch_bounds__(kLbaBlock) void k_lba_gather_points(LbaView V, const float* wpos, const int32_t* slot) {
  const int p = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (p >= V.nP) return;
  for (int i = 0; i < 3; ++i) V.X[3 * (size_t)p + i] = V.Xt[3 * (size_t)p + i] = (double)wpos[3 * (size_t)slot[p] + i];
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_linearise(LbaView V) {
  const int k = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (k < V.nE) lba_linearise_edge(V, k);
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_point_sums(LbaView V) {
  const int p = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (p < V.nP) lba_point_sums(V, p);
}
__global__ __launch_bounds__(kLbaCamLanes) void k_lba_cam_blocks(LbaView V) {
  const int a = (int)blockIdx.x, lane = (int)threadIdx.x;
  double acc[27];
  lba_cam_lane(V, a, lane, acc);
  for (int s = kLbaCamLanes / 2; s >= 1; s >>= 1) {
#pragma unroll
    for (int c = 0; c < 27; ++c) acc[c] = acc[c] + __shfl_down(acc[c], (unsigned)s);   // lanes >= s form sums nobody reads
  }
  if (lane == 0) {
    for (int c = 0; c < 21; ++c) V.cam_H[21 * (size_t)a + c] = acc[c];
    for (int c = 0; c < 6; ++c) V.cam_b[6 * (size_t)a + c] = acc[21 + c];
  }
}
// mode 0, after the linearisation: chi and maxdiag; mode 1, after a trial: chi and scale
__global__ __launch_bounds__(kLmLanes) void k_lba_sums(LbaView V, int mode, double lambda) {
  __shared__ double s_v[2][kLmLanes];
  const int tid = (int)threadIdx.x;
  s_v[0][tid] = lba_sum_lane(V, 0, lambda, tid);
  s_v[1][tid] = lba_sum_lane(V, mode == 0 ? 2 : 1, lambda, tid);
  __syncthreads();
  for (int s = kLmLanes / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      s_v[0][tid] = s_v[0][tid] + s_v[0][tid + s];
      s_v[1][tid] = mode == 0 ? lba_max(s_v[1][tid], s_v[1][tid + s]) : s_v[1][tid] + s_v[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    V.rec->chi = s_v[0][0];
    if (mode == 0) V.rec->maxdiag = s_v[1][0]; else V.rec->scale = s_v[1][0];
  }
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_trial_edges(LbaView V, double lambda) {
  const int k = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (k < V.nE) lba_trial_edge(V, lambda, k);
}
// grid = (column j, column i): the blocks below the diagonal leave at once
__global__ __launch_bounds__(kLbaSchurLanes) void k_lba_schur(LbaView V, double lambda) {
  const int j = (int)blockIdx.x, i = (int)blockIdx.y;
  if (i <= j) lba_schur_lane(V, lambda, i, j, (int)threadIdx.x);
}

// (S + lambda I) x = b_schur: lm_solve_n's elements, whole elements in parallel.  Work-item t owns the rows t, t + 256, ...
// Column j: row j goes to LDS; every row i >= j forms a_ij - sum_p (L_ip L_jp) D_p; after a barrier all read the pivot, rows
// i > j divide.  Forward substitution sweeps the columns (y_p final, every row below subtracts L_ip y_p: p ascending per
// element); the backward one is lm_solve's ascending sum per row, which needs every x below it first - work-item 0 runs it.
// Every loop is bounded by n <= 768; every work-item reaches every barrier (the pivot test is uniform).
__global__ __launch_bounds__(kLmLanes) void k_lba_factor(LbaView V) {
  __shared__ double s_tri[kLbaLdsN * (kLbaLdsN + 1) / 2];
  __shared__ double s_D[6 * kLbaMaxFree], s_y[6 * kLbaMaxFree], s_row[6 * kLbaMaxFree];
  const int tid = (int)threadIdx.x, n = V.n;
  const size_t tri = lm_tri((size_t)n, 0);
  double* A = V.S;
  if (n <= kLbaLdsN) {
    for (size_t q = (size_t)tid; q < tri; q += kLmLanes) s_tri[q] = V.S[q];
    A = s_tri;
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < n && ok; ++j) {
    const double* Lj = A + lm_tri((size_t)j, 0);
    for (int p = tid; p < j; p += kLmLanes) s_row[p] = Lj[p];
    __syncthreads();
    for (int i = j + tid; i < n; i += kLmLanes) {
      double* Li = A + lm_tri((size_t)i, 0);
      double v = Li[j];
      for (int p = 0; p < j; ++p) v = v - Li[p] * s_row[p] * s_D[p];
      Li[j] = v;
    }
    __syncthreads();
    const double d = Lj[j];
    ok = d > 0.0 && d <= DBL_MAX;
    if (ok) {
      if (tid == 0) s_D[j] = d;
      for (int i = j + 1 + tid; i < n; i += kLmLanes) A[lm_tri((size_t)i, (size_t)j)] = A[lm_tri((size_t)i, (size_t)j)] / d;
    }
    __syncthreads();
  }
  if (ok) {
    for (int i = tid; i < n; i += kLmLanes) s_y[i] = V.bs[i];
    __syncthreads();
    for (int p = 0; p < n; ++p) {
      const double yp = s_y[p];
      for (int i = p + 1 + tid; i < n; i += kLmLanes) s_y[i] = s_y[i] - A[lm_tri((size_t)i, (size_t)p)] * yp;
      __syncthreads();
    }
    for (int i = tid; i < n; i += kLmLanes) s_y[i] = s_y[i] / s_D[i];
    __syncthreads();
    if (tid == 0) {
      for (int i = n - 1; i >= 0; --i) {   // x in s_row: the staged rows are not read again
        double v = s_y[i];
        for (int p = i + 1; p < n; ++p) v = v - A[lm_tri((size_t)p, (size_t)i)] * s_row[p];
        s_row[i] = v;
      }
    }
    __syncthreads();
  }
  for (int a = tid; a < V.nA; a += kLmLanes) {
    if (ok)
      for (int r = 0; r < 6; ++r) V.x_cam[6 * (size_t)a + r] = s_row[6 * a + r];
    lba_trial_camera(V, a);   // after a failed factorisation: the x the cameras hold
  }
  if (tid == 0) V.rec->ok = ok ? 1 : 0;
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_trial_points(LbaView V, double lambda) {
  const int r = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (r < V.nPa) lba_trial_point(V, lambda, V.rec->ok != 0, V.act_pt[r]);
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_flags(LbaView V) {
  const int k = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (k < V.nE) lba_flag_edge(V, k);
}
__global__ __launch_bounds__(kLbaBlock) void k_lba_pool_write(LbaView V, float* wpos, const int32_t* slot) {
  const int p = (int)(blockIdx.x * kLbaBlock + threadIdx.x);
  if (p >= V.nP) return;
  for (int i = 0; i < 3; ++i) wpos[3 * (size_t)slot[p] + i] = (float)V.X[3 * (size_t)p + i];
}

}  // namespace rgbl

using namespace rgbl;

using namespace rgbl_lba;

int rgbl_local_bundle_adjustment_host(const rgbl_lba_input* in, rgbl_lba_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  LbaProblem P;
  RGBL_TRY(check_lba_input(in, true, P));
  RGBL_TRY(build_lba_structure(in, P));
  LbaStop stop = {in->stop, in->stop_byte, in->stop_after_polls, 0};
  if (lba_returns_early(P, stop)) { write_lba_early(out, stop); return RGBL_OK; }
  P.X.resize(3 * (size_t)P.nP);
  for (size_t i = 0; i < P.X.size(); ++i) P.X[i] = (double)in->world_pos[i];   // :1286
  const LbaOffsets O = lba_offsets(P);
  std::vector<uint8_t> mem(O.total, 0);
  lba_fill(in, P, O, [&](size_t off, const void* src, size_t bytes) { if (bytes) memcpy(mem.data() + off, src, bytes); });
  LbaHostBackend B;
  B.V = lba_view(P, O, mem.data());
  B.D.resize((size_t)B.V.n); B.y.resize((size_t)B.V.n);
  LbaCounters D;
  lm_levenberg_loop(B, P.nE > 0 ? in->max_iterations : 0, in->user_lambda_init, stop, D);
  for (int k = 0; k < P.nE; ++k) lba_flag_edge(B.V, k);
  write_lba_output(in, out, P, B.V.T, B.V.X, B.V.e_chi2, B.V.flags, D, stop);
  return RGBL_OK;
}

int rgbl_local_bundle_adjustment(rgbl_matcher* m, const rgbl_lba_input* in, rgbl_lba_output* out) {
  if (!m || !in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  LbaProblem P;
  RGBL_TRY(check_lba_input(in, false, P));
  PoolCall pc(m, "local BA", "a frame");
  RGBL_TRY(pc.note(in->pool, {}, -1));
  RGBL_TRY(pc.lock(1, [&](int) -> int { return check_lba_slots(pc, in->slot, P); }));
  float* d_wpos = pc.pool ? pc.pool->d_wpos : nullptr;
  RGBL_TRY(build_lba_structure(in, P));
  LbaStop stop = {in->stop, in->stop_byte, in->stop_after_polls, 0};
  if (lba_returns_early(P, stop)) { write_lba_early(out, stop); return RGBL_OK; }
  if (!in->pool) {
    P.X.resize(3 * (size_t)P.nP);
    for (size_t i = 0; i < P.X.size(); ++i) P.X[i] = (double)in->world_pos[i];   // :1286
  }
  const LbaOffsets O = lba_offsets(P);
  // the page-locked side: the record, then what comes back (T | X | e_chi2 | flags)
  const size_t back_begin = O.T, back_end = O.flags + (size_t)P.nE, pin_back = 256;
  RGBL_HIP(hipSetDevice(m->device));
  RGBL_TRY(ensure_arena(m, O.total));
  RGBL_TRY(ensure_pin(m, pin_back + (back_end - back_begin)));
  LbaDeviceBackend B;
  B.m = m; B.s = m->stream;
  uint8_t *d_buf = m->d_buf, *h_pin = m->h_pin;
  StreamDrain drain(B.s);   // behind pc (PoolCall): the stream is idle before the pool is released
  B.V = lba_view(P, O, d_buf);
  B.h_rec = reinterpret_cast<LbaRecord*>(h_pin);
  RGBL_HIP(hipMemsetAsync(d_buf, 0, O.total, B.s));
  int rc = RGBL_OK;
  lba_fill(in, P, O, [&](size_t off, const void* src, size_t bytes) {
    if (!bytes || rc != RGBL_OK) return;
    const hipError_t e = hipMemcpyAsync(d_buf + off, src, bytes, hipMemcpyHostToDevice, B.s);   // pageable sources: staged by the runtime before it returns
    if (e != hipSuccess) { set_error("local BA: upload: %s", hipGetErrorString(e)); rc = RGBL_ERR_HIP; }
  });
  RGBL_TRY(rc);
  const int32_t* d_slot = reinterpret_cast<const int32_t*>(d_buf + O.slot);
  if (in->pool && P.nP > 0) B.launch("k_lba_gather_points", k_lba_gather_points, dim3(B.blocks(P.nP)), dim3(kLbaBlock), B.V, (const float*)d_wpos, d_slot);
  LbaCounters D;
  const bool done = lm_levenberg_loop(B, P.nE > 0 ? in->max_iterations : 0, in->user_lambda_init, stop, D);
  if (!done) return B.rc;
  if (P.nE > 0) B.launch("k_lba_flags", k_lba_flags, dim3(B.blocks(P.nE)), dim3(kLbaBlock), B.V);
  if (in->pool && P.nP > 0) B.launch("k_lba_pool_write", k_lba_pool_write, dim3(B.blocks(P.nP)), dim3(kLbaBlock), B.V, d_wpos, d_slot);
  RGBL_TRY(B.rc);
  RGBL_HIP(hipMemcpyAsync(h_pin + pin_back, d_buf + back_begin, back_end - back_begin, hipMemcpyDeviceToHost, B.s));
  RGBL_HIP(hipStreamSynchronize(B.s));
  m->timer.collect();
  const uint8_t* back = h_pin + pin_back - back_begin;
  write_lba_output(in, out, P, reinterpret_cast<const PoPose*>(back + O.T), reinterpret_cast<const double*>(back + O.X),
                   reinterpret_cast<const double*>(back + O.e_chi2), back + O.flags, D, stop);
  return RGBL_OK;
}
