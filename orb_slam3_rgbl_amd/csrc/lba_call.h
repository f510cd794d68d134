// lba_call.h — the call scaffold of the bundle adjustments, shared by lba.hip (LocalBundleAdjustment) and gba.hip
// (BundleAdjustment): the problem as both builds read it, its checks, the lists the kernels walk, the one layout of the
// host's vectors and the device's arena, and the two executions of lm_levenberg_loop's passes.  The per-item kernels are
// defined in lba.hip and launched from both files.  Private to csrc; included after common.h and matcher_call.h.
#pragma once
#include <string.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "matcher_call.h"
#include "lba_math.h"

namespace rgbl {

constexpr int kLbaBlock = 64;   // work-items of the per-edge and per-point kernels (fp64 throughout: registers, not occupancy)

__global__ void k_lba_gather_points(LbaView V, const float* wpos, const int32_t* slot);
__global__ void k_lba_linearise(LbaView V);
__global__ void k_lba_point_sums(LbaView V);
__global__ void k_lba_cam_blocks(LbaView V);
__global__ void k_lba_sums(LbaView V, int mode, double lambda);
__global__ void k_lba_trial_edges(LbaView V, double lambda);
__global__ void k_lba_schur(LbaView V, double lambda);
__global__ void k_lba_factor(LbaView V);
__global__ void k_lba_trial_points(LbaView V, double lambda);
__global__ void k_lba_flags(LbaView V);
__global__ void k_lba_pool_write(LbaView V, float* wpos, const int32_t* slot);

}  // namespace rgbl

namespace rgbl_lba {
using namespace rgbl;

// The call as both builds read it: what the caller gave, the active set and the structure of the reduced system.
struct LbaProblem {
  // the entry point: its name in the error texts, how many cameras the free list may hold and how many may be active, whether
  // the edges have their Huber kernel, and whether the reduced system goes to the panel solve (csrc/gba.hip)
  const char* what = "local BA";
  int max_listed = kLbaMaxFree, max_active = kLbaMaxFree;
  bool robust = true, panel = false;
  double delta[2] = {po_delta(false), po_delta(true)};   // thHuberMono, thHuberStereo of :1275-1276; BundleAdjustment sets its own
  int nC = 0, nA = 0, nP = 0, nE = 0, nPa = 0, n_fixed_total = 0;
  std::vector<int32_t> blk_list;   // panel: the upper blocks (i, j) that are not empty - every diagonal one, the others with a pair
  std::vector<PoPose> T;
  std::vector<PoCam> C;
  std::vector<int32_t> col, col_cam, pt_off, act_pt, cam_eoff, cam_edges, blk_off, pairs;
  std::vector<double> X;
};

// everything that can be refused is refused here, before anything is uploaded, launched or written
inline int check_lba_input(const rgbl_lba_input* in, bool host_only, LbaProblem& P) {
  if (P.panel && (in->n_free < 0 || in->n_free > P.max_listed)) { set_error("%s: n_cams outside [0, %d]", P.what, P.max_listed); return RGBL_ERR_INVALID; }   // BundleAdjustment's one list
  if (in->n_free < 0 || in->n_free > P.max_listed || in->n_fixed < 0 || in->n_fixed > kLbaMaxFixed) { set_error("%s: n_free outside [0, %d] or n_fixed outside [0, %d]", P.what, P.max_listed, kLbaMaxFixed); return RGBL_ERR_INVALID; }
  if (in->n_points < 0 || in->n_points > kLbaMaxPoints || in->n_edges < 0 || in->n_edges > kLbaMaxEdges) { set_error("%s: n_points outside [0, %d] or n_edges outside [0, %d]", P.what, kLbaMaxPoints, kLbaMaxEdges); return RGBL_ERR_INVALID; }
  const int nC = in->n_free + in->n_fixed, nP = in->n_points, nE = in->n_edges;
  if (nC > 0 && (!in->cam_q || !in->cam_t || !in->cam_K || !in->cam_bf)) { set_error("%s: no cam_q / cam_t / cam_K / cam_bf", P.what); return RGBL_ERR_INVALID; }
  if (host_only && in->pool) { set_error("%s: the host build reads host arrays only", P.what); return RGBL_ERR_INVALID; }
  if (nP > 0 && (in->pool ? !in->slot : !in->world_pos)) { set_error("%s: the points are either world_pos or a pool with slot", P.what); return RGBL_ERR_INVALID; }
  if (nE > 0 && (!in->edge_point || !in->edge_cam || !in->edge_obs || !in->edge_inv_sigma2)) { set_error("%s: no edge_point / edge_cam / edge_obs / edge_inv_sigma2", P.what); return RGBL_ERR_INVALID; }
  bool finite = true;
  for (int c = 0; c < nC; ++c) {
    finite = finite && std::isfinite(in->cam_bf[c]);
    for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->cam_q[4 * (size_t)c + i]) && std::isfinite(in->cam_K[4 * (size_t)c + i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(in->cam_t[3 * (size_t)c + i]);
  }
  if (!finite) { set_error("%s: a pose, K or bf is not finite", P.what); return RGBL_ERR_INVALID; }
  for (int c = 0; c < nC; ++c) {
    const float* q = in->cam_q + 4 * (size_t)c;
    if (q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 0.0f) { set_error("%s: camera %d has an all-zero quaternion", P.what, c); return RGBL_ERR_INVALID; }
  }
  std::vector<int32_t> seen((size_t)nC, -1), n_cam_edges((size_t)nC, 0);
  P.pt_off.assign((size_t)nP + 1, 0);
  for (int k = 0; k < nE; ++k) {
    const int p = in->edge_point[k], c = in->edge_cam[k];
    if (p < 0 || p >= nP || c < 0 || c >= nC) { set_error("%s: edge %d names point %d of %d, camera %d of %d", P.what, k, p, nP, c, nC); return RGBL_ERR_INVALID; }
    if (k > 0 && p < in->edge_point[k - 1]) { set_error("%s: edge_point decreases at edge %d", P.what, k); return RGBL_ERR_INVALID; }
    if (seen[(size_t)c] == p) { set_error("%s: edge %d repeats the pair (point %d, camera %d)", P.what, k, p, c); return RGBL_ERR_INVALID; }
    seen[(size_t)c] = p;
    ++n_cam_edges[(size_t)c];
    ++P.pt_off[(size_t)p + 1];
  }
  for (int p = 0; p < nP; ++p) P.pt_off[(size_t)p + 1] += P.pt_off[(size_t)p];
  P.nC = nC; P.nP = nP; P.nE = nE;
  P.n_fixed_total = in->n_fixed;
  // the active set (g2o's initializeOptimization): a vertex an edge touches
  P.col.assign((size_t)nC, -1);
  for (int c = 0; c < in->n_free; ++c) {
    const bool fixed = in->free_is_fixed && in->free_is_fixed[c];
    if (fixed) ++P.n_fixed_total;
    if (!fixed && n_cam_edges[(size_t)c] > 0) { P.col[(size_t)c] = (int32_t)P.col_cam.size(); P.col_cam.push_back(c); }
  }
  P.nA = (int)P.col_cam.size();
  // BundleAdjustment lists every camera as free: what it flags fixed keeps LBA's bound on fixed cameras, what is active its own
  if (P.panel && (P.nA > P.max_active || P.n_fixed_total > kLbaMaxFixed)) { set_error("%s: %d active free cameras of at most %d, %d fixed ones of at most %d", P.what, P.nA, P.max_active, P.n_fixed_total, kLbaMaxFixed); return RGBL_ERR_INVALID; }
  for (int p = 0; p < nP; ++p)
    if (P.pt_off[(size_t)p + 1] > P.pt_off[(size_t)p]) P.act_pt.push_back(p);
  P.nPa = (int)P.act_pt.size();
  P.T.resize((size_t)nC);
  P.C.resize((size_t)nC);
  for (int c = 0; c < nC; ++c) {
    P.T[(size_t)c] = po_pose_from_float(in->cam_q + 4 * (size_t)c, in->cam_t + 3 * (size_t)c);   // :1218 / :1235
    const float* K = in->cam_K + 4 * (size_t)c;
    P.C[(size_t)c] = PoCam{(double)K[0], (double)K[1], (double)K[2], (double)K[3], (double)in->cam_bf[c]};
  }
  return RGBL_OK;
}

// under the pool's lock: the smallest slot below 0, else the largest beyond the pool, else the first listed twice
inline int check_lba_slots(const PoolCall& pc, const int32_t* slot, const LbaProblem& P) {
  std::vector<int32_t> sorted(slot, slot + P.nP);
  std::sort(sorted.begin(), sorted.end());
  if (P.nP > 0 && !(pc.holds(sorted.front()) && pc.holds(sorted.back()))) { set_error("%s: slot %d outside [0, %d)", P.what, sorted.front() < 0 ? sorted.front() : sorted.back(), pc.pool->cap); return RGBL_ERR_INVALID; }
  for (int p = 0; p + 1 < P.nP; ++p)
    if (sorted[(size_t)p] == sorted[(size_t)p + 1]) { set_error("%s: slot %d is listed twice", P.what, sorted[(size_t)p]); return RGBL_ERR_INVALID; }
  return RGBL_OK;
}

// the lists the kernels walk; built once per call (the structure does not change between iterations)
inline int build_lba_structure(const rgbl_lba_input* in, LbaProblem& P) {
  const int nA = P.nA, nE = P.nE;
  P.cam_eoff.assign((size_t)nA + 1, 0);
  for (int k = 0; k < nE; ++k) {
    const int a = P.col[(size_t)in->edge_cam[k]];
    if (a >= 0) ++P.cam_eoff[(size_t)a + 1];
  }
  for (int a = 0; a < nA; ++a) P.cam_eoff[(size_t)a + 1] += P.cam_eoff[(size_t)a];
  P.cam_edges.resize((size_t)P.cam_eoff[(size_t)nA]);
  std::vector<int32_t> fill(P.cam_eoff.begin(), P.cam_eoff.end() - 1);
  for (int k = 0; k < nE; ++k) {
    const int a = P.col[(size_t)in->edge_cam[k]];
    if (a >= 0) P.cam_edges[(size_t)fill[(size_t)a]++] = k;
  }
  const int nB = nA * (nA + 1) / 2;
  std::vector<int64_t> count((size_t)nB + 1, 0);
  auto each_pair = [&](auto&& f) {
    for (int p = 0; p < P.nP; ++p)
      for (int k1 = P.pt_off[(size_t)p]; k1 < P.pt_off[(size_t)p + 1]; ++k1) {
        const int a1 = P.col[(size_t)in->edge_cam[k1]];
        if (a1 < 0) continue;
        for (int k2 = P.pt_off[(size_t)p]; k2 < P.pt_off[(size_t)p + 1]; ++k2) {
          const int a2 = P.col[(size_t)in->edge_cam[k2]];
          if (a2 >= a1) f(lba_block(nA, a1, a2), k1, k2);
        }
      }
  };
  each_pair([&](int blk, int, int) { ++count[(size_t)blk + 1]; });
  for (int b = 0; b < nB; ++b) count[(size_t)b + 1] += count[(size_t)b];
  // at most 128 active cameras per point and 2^20 edges: fewer than 2^27 pairs, an int32 holds every offset.  With 1 024
  // active cameras a call could reach 2^29; beyond 2^27 (1 GiB of pairs) it is refused
  if (count[(size_t)nB] > ((int64_t)1 << 27)) { set_error("%s: more than 2^27 pairs of edges that share a point", P.what); return RGBL_ERR_INVALID; }
  if (P.panel)
    for (int i = 0; i < nA; ++i)
      for (int j = i; j < nA; ++j) {
        const int blk = lba_block(nA, i, j);
        if (i == j || count[(size_t)blk + 1] > count[(size_t)blk]) { P.blk_list.push_back(i); P.blk_list.push_back(j); }
      }
  P.blk_off.resize((size_t)nB + 1);
  for (int b = 0; b <= nB; ++b) P.blk_off[(size_t)b] = (int32_t)count[(size_t)b];
  P.pairs.resize(2 * (size_t)count[(size_t)nB]);
  std::vector<int32_t> at(P.blk_off.begin(), P.blk_off.end() - 1);
  each_pair([&](int blk, int k1, int k2) {
    const size_t q = (size_t)at[(size_t)blk]++;
    P.pairs[2 * q] = k1; P.pairs[2 * q + 1] = k2;
  });
  return RGBL_OK;
}

// poll 1 (:1406-1408) and :1182-1186
inline bool lba_returns_early(const LbaProblem& P, LbaStop& stop) {
  if (P.n_fixed_total == 0) return true;
  return stop.poll();
}

inline void write_lba_early(rgbl_lba_output* out, const LbaStop& stop) {
  double *q = out->diag.cam_q, *t = out->diag.cam_t, *x = out->diag.point;
  memset(&out->diag, 0, sizeof(out->diag));
  out->diag.cam_q = q; out->diag.cam_t = t; out->diag.point = x;
  out->diag.polls = stop.polls;
}

inline void write_lba_output(const rgbl_lba_input* in, rgbl_lba_output* out, const LbaProblem& P, const PoPose* T, const double* X,
                      const double* chi2, const uint8_t* flags, const LbaCounters& D, const LbaStop& stop) {
  for (int c = 0; c < in->n_free; ++c) {
    for (int i = 0; i < 4; ++i) {
      if (out->cam_q) out->cam_q[4 * (size_t)c + i] = (float)T[c].q[i];   // :1484
      if (out->diag.cam_q) out->diag.cam_q[4 * (size_t)c + i] = T[c].q[i];
    }
    for (int i = 0; i < 3; ++i) {
      if (out->cam_t) out->cam_t[3 * (size_t)c + i] = (float)T[c].t[i];
      if (out->diag.cam_t) out->diag.cam_t[3 * (size_t)c + i] = T[c].t[i];
    }
  }
  for (size_t i = 0; i < 3 * (size_t)P.nP; ++i) {
    if (out->point) out->point[i] = (float)X[i];   // :1493
    if (out->diag.point) out->diag.point[i] = X[i];
  }
  if (out->chi2 && P.nE) memcpy(out->chi2, chi2, sizeof(double) * (size_t)P.nE);
  if (out->flags && P.nE) memcpy(out->flags, flags, (size_t)P.nE);
  rgbl_lba_diag& G = out->diag;
  G.ran = 1; G.iterations = D.iterations; G.trials = D.trials; G.rejected = D.rejected; G.failed = D.failed;
  G.active_cams = P.nA; G.active_points = P.nPa; G.polls = stop.polls;
  G.first_chi2 = D.first_chi2; G.last_chi2 = D.last_chi2; G.last_lambda = D.last_lambda;
}

// the host's execution of the passes
struct LbaHostBackend {
  LbaView V;
  std::vector<double> D, y;
  bool panel = false;   // the reduced system goes to lm_solve_panel (BundleAdjustment): the backward order is the mirrored one
  bool linearise(bool, double* chi, double* maxdiag) {
    for (int k = 0; k < V.nE; ++k) lba_linearise_edge(V, k);
    for (int p = 0; p < V.nP; ++p) lba_point_sums(V, p);
    std::vector<double> part((size_t)kLbaCamLanes * 27);
    for (int a = 0; a < V.nA; ++a) {
      for (int l = 0; l < kLbaCamLanes; ++l) lba_cam_lane(V, a, l, &part[(size_t)l * 27]);
      for (int s = kLbaCamLanes / 2; s >= 1; s >>= 1)
        for (int i = 0; i < s; ++i)
          for (int c = 0; c < 27; ++c) part[(size_t)i * 27 + c] = part[(size_t)i * 27 + c] + part[(size_t)(i + s) * 27 + c];
      for (int c = 0; c < 21; ++c) V.cam_H[21 * (size_t)a + c] = part[(size_t)c];
      for (int c = 0; c < 6; ++c) V.cam_b[6 * (size_t)a + c] = part[21 + (size_t)c];
    }
    *chi = tree(0, 0.0, false);
    *maxdiag = tree(2, 0.0, true);
    return true;
  }
  double tree(int what, double lambda, bool is_max) {
    double v[kLmLanes];
    for (int l = 0; l < kLmLanes; ++l) v[l] = lba_sum_lane(V, what, lambda, l);
    for (int s = kLmLanes / 2; s >= 1; s >>= 1)
      for (int i = 0; i < s; ++i) v[i] = is_max ? lba_max(v[i], v[i + s]) : v[i] + v[i + s];
    return v[0];
  }
  bool trial(double lambda, bool* ok, double* chi, double* scale) {
    for (int k = 0; k < V.nE; ++k) lba_trial_edge(V, lambda, k);
    for (int i = 0; i < V.nA; ++i)
      for (int j = i; j < V.nA; ++j)
        for (int t = 0; t < 42; ++t) lba_schur_lane(V, lambda, i, j, t);
    std::vector<double> x((size_t)V.n);
    *ok = panel ? lm_solve_panel(V.n, kLmPanel, V.S, V.bs, x.data(), D.data(), y.data()) : lm_solve_n(V.n, V.S, V.bs, x.data(), D.data(), y.data());
    if (*ok)
      for (int u = 0; u < V.n; ++u) V.x_cam[u] = x[(size_t)u];
    for (int a = 0; a < V.nA; ++a) lba_trial_camera(V, a);
    for (int r = 0; r < V.nPa; ++r) lba_trial_point(V, lambda, *ok, V.act_pt[r]);
    *chi = tree(0, lambda, false);
    *scale = tree(1, lambda, false);
    return true;
  }
  bool accept() {
    for (int c = 0; c < V.nC; ++c) V.T[c] = V.Tt[c];
    for (size_t i = 0; i < 3 * (size_t)V.nP; ++i) V.X[i] = V.Xt[i];
    return true;
  }
};

// the arrays of a view, in one order for the host's vectors and the device's arena
struct LbaLayout {
  size_t off = 0;
  template <class E> size_t take(size_t count) {
    off = (off + 255) / 256 * 256;
    const size_t at = off;
    off += count * sizeof(E);
    return at;
  }
};
struct LbaOffsets {
  size_t T, Tt, C, col, col_cam, X, Xt, pt_off, act_pt, e_pt, e_cam, e_obs, e_info, e_chi2, e_rho, lin, tr, cam_eoff, cam_edges,
      blk_off, pairs, pt_H, pt_b, cam_H, cam_b, S, bs, x_cam, x_pt, rec, flags, slot, blk_list, pD, py, pyf, pxw, pfail, total;
};
inline LbaOffsets lba_offsets(const LbaProblem& P) {
  LbaLayout L;
  LbaOffsets O;
  const size_t nC = (size_t)P.nC, nA = (size_t)P.nA, nP = (size_t)P.nP, nE = (size_t)P.nE, n = 6 * nA;
  // what the call downloads lies side by side: T | X | e_chi2 | flags
  O.T = L.take<PoPose>(nC); O.X = L.take<double>(3 * nP); O.e_chi2 = L.take<double>(nE); O.flags = L.take<uint8_t>(nE);
  O.Tt = L.take<PoPose>(nC); O.C = L.take<PoCam>(nC); O.col = L.take<int32_t>(nC); O.col_cam = L.take<int32_t>(nA);
  O.Xt = L.take<double>(3 * nP); O.pt_off = L.take<int32_t>(nP + 1); O.act_pt = L.take<int32_t>((size_t)P.nPa);
  O.e_pt = L.take<int32_t>(nE); O.e_cam = L.take<int32_t>(nE); O.e_obs = L.take<float>(3 * nE); O.e_info = L.take<float>(nE);
  O.e_rho = L.take<double>(nE); O.lin = L.take<LbaEdgeLin>(nE); O.tr = L.take<LbaEdgeTrial>(nE);
  O.cam_eoff = L.take<int32_t>(nA + 1); O.cam_edges = L.take<int32_t>(P.cam_edges.size());
  O.blk_off = L.take<int32_t>(P.blk_off.size()); O.pairs = L.take<int32_t>(P.pairs.size());
  O.pt_H = L.take<double>(6 * nP); O.pt_b = L.take<double>(3 * nP); O.cam_H = L.take<double>(21 * nA); O.cam_b = L.take<double>(6 * nA);
  O.S = L.take<double>(lm_tri(n, 0)); O.bs = L.take<double>(n); O.x_cam = L.take<double>(n); O.x_pt = L.take<double>(3 * nP);
  O.rec = L.take<LbaRecord>(1); O.slot = L.take<int32_t>(nP);
  // the panel solve's vectors (csrc/gba.hip); nothing for LocalBundleAdjustment
  const size_t np = P.panel ? n : 0;
  O.blk_list = L.take<int32_t>(P.blk_list.size()); O.pD = L.take<double>(np); O.py = L.take<double>(np); O.pyf = L.take<double>(np);
  O.pxw = L.take<double>(np); O.pfail = L.take<int32_t>(P.panel ? 1 : 0);
  O.total = (L.off + 255) / 256 * 256;
  return O;
}
inline LbaView lba_view(const LbaProblem& P, const LbaOffsets& O, uint8_t* base) {
  LbaView V;
  V.nC = P.nC; V.nA = P.nA; V.nP = P.nP; V.nE = P.nE; V.nPa = P.nPa; V.n = 6 * P.nA;
  V.robust = P.robust ? 1 : 0;
  V.delta[0] = P.delta[0]; V.delta[1] = P.delta[1];
  auto at = [&](size_t off) { return base + off; };
  V.T = (PoPose*)at(O.T); V.Tt = (PoPose*)at(O.Tt); V.C = (const PoCam*)at(O.C);
  V.col = (const int32_t*)at(O.col); V.col_cam = (const int32_t*)at(O.col_cam);
  V.X = (double*)at(O.X); V.Xt = (double*)at(O.Xt); V.pt_off = (const int32_t*)at(O.pt_off); V.act_pt = (const int32_t*)at(O.act_pt);
  V.e_pt = (const int32_t*)at(O.e_pt); V.e_cam = (const int32_t*)at(O.e_cam); V.e_obs = (const float*)at(O.e_obs);
  V.e_info = (const float*)at(O.e_info); V.e_chi2 = (double*)at(O.e_chi2); V.e_rho = (double*)at(O.e_rho);
  V.lin = (LbaEdgeLin*)at(O.lin); V.tr = (LbaEdgeTrial*)at(O.tr);
  V.cam_eoff = (const int32_t*)at(O.cam_eoff); V.cam_edges = (const int32_t*)at(O.cam_edges);
  V.blk_off = (const int32_t*)at(O.blk_off); V.pairs = (const int32_t*)at(O.pairs);
  V.pt_H = (double*)at(O.pt_H); V.pt_b = (double*)at(O.pt_b); V.cam_H = (double*)at(O.cam_H); V.cam_b = (double*)at(O.cam_b);
  V.S = (double*)at(O.S); V.bs = (double*)at(O.bs); V.x_cam = (double*)at(O.x_cam); V.x_pt = (double*)at(O.x_pt);
  V.rec = (LbaRecord*)at(O.rec); V.flags = at(O.flags);
  V.blk_list = (const int32_t*)at(O.blk_list); V.n_blk_list = (int)(P.blk_list.size() / 2);
  V.pD = (double*)at(O.pD); V.py = (double*)at(O.py); V.pyf = (double*)at(O.pyf); V.pxw = (double*)at(O.pxw); V.pfail = (int32_t*)at(O.pfail);
  return V;
}
// what a build starts from, written through `put(offset, source, bytes)`; everything else starts as zeros
template <class Put> void lba_fill(const rgbl_lba_input* in, const LbaProblem& P, const LbaOffsets& O, Put put) {
  const size_t nC = (size_t)P.nC, nP = (size_t)P.nP, nE = (size_t)P.nE;
  put(O.T, P.T.data(), nC * sizeof(PoPose)); put(O.Tt, P.T.data(), nC * sizeof(PoPose)); put(O.C, P.C.data(), nC * sizeof(PoCam));
  put(O.col, P.col.data(), nC * 4); put(O.col_cam, P.col_cam.data(), P.col_cam.size() * 4);
  if (!in->pool) { put(O.X, P.X.data(), nP * 24); put(O.Xt, P.X.data(), nP * 24); }
  else put(O.slot, in->slot, nP * 4);
  put(O.pt_off, P.pt_off.data(), (nP + 1) * 4); put(O.act_pt, P.act_pt.data(), P.act_pt.size() * 4);
  put(O.e_pt, in->edge_point, nE * 4); put(O.e_cam, in->edge_cam, nE * 4); put(O.e_obs, in->edge_obs, nE * 12);
  put(O.e_info, in->edge_inv_sigma2, nE * 4);
  put(O.cam_eoff, P.cam_eoff.data(), P.cam_eoff.size() * 4); put(O.cam_edges, P.cam_edges.data(), P.cam_edges.size() * 4);
  put(O.blk_off, P.blk_off.data(), P.blk_off.size() * 4); put(O.pairs, P.pairs.data(), P.pairs.size() * 4);
  put(O.blk_list, P.blk_list.data(), P.blk_list.size() * 4);
}

// the device's execution of the passes: launches on the matcher's stream, one record read back per pass
struct LbaDeviceBackend {
  LbaView V;
  rgbl_matcher* m;
  hipStream_t s;
  LbaRecord* h_rec;   // page-locked
  int rc = RGBL_OK;   // the first error of a launch or a copy; nothing is launched behind it
  const char* what = "local BA";   // the entry point in the error texts
  // the reduced system of a trial: null, LocalBundleAdjustment's k_lba_schur over every block and k_lba_factor; csrc/gba.hip sets
  // its launches over the blocks that are not empty and the panel solve
  void (*reduced)(LbaDeviceBackend&, double lambda) = nullptr;
  static unsigned blocks(int items) { return (unsigned)((items + kLbaBlock - 1) / kLbaBlock); }
  template <class... Params, class... Args> void launch(const char* name, void (*k)(Params...), dim3 grid, dim3 block, const Args&... args) {
    if (rc == RGBL_OK) rc = rgbl::launch(m, s, name, k, grid, block, 0, args...);
  }
  int fetch() {
    RGBL_TRY(rc);
    RGBL_HIP(hipMemcpyAsync(h_rec, V.rec, sizeof(LbaRecord), hipMemcpyDeviceToHost, s));
    RGBL_HIP(hipStreamSynchronize(s));
    m->timer.collect();
    return RGBL_OK;
  }
  bool linearise(bool, double* chi, double* maxdiag) {
    launch("k_lba_linearise", k_lba_linearise, dim3(blocks(V.nE)), dim3(kLbaBlock), V);
    launch("k_lba_point_sums", k_lba_point_sums, dim3(blocks(V.nP)), dim3(kLbaBlock), V);
    if (V.nA > 0) launch("k_lba_cam_blocks", k_lba_cam_blocks, dim3((unsigned)V.nA), dim3(kLbaCamLanes), V);
    launch("k_lba_sums", k_lba_sums, dim3(1), dim3(kLmLanes), V, 0, 0.0);
    rc = fetch();
    *chi = h_rec->chi; *maxdiag = h_rec->maxdiag;
    return rc == RGBL_OK;
  }
  bool trial(double lambda, bool* ok, double* chi, double* scale) {
    launch("k_lba_trial_edges", k_lba_trial_edges, dim3(blocks(V.nE)), dim3(kLbaBlock), V, lambda);
    if (reduced) reduced(*this, lambda);
    else {
      if (V.nA > 0) launch("k_lba_schur", k_lba_schur, dim3((unsigned)V.nA, (unsigned)V.nA), dim3(kLbaSchurLanes), V, lambda);
      launch("k_lba_factor", k_lba_factor, dim3(1), dim3(kLmLanes), V);
    }
    launch("k_lba_trial_points", k_lba_trial_points, dim3(blocks(V.nPa)), dim3(kLbaBlock), V, lambda);
    launch("k_lba_sums", k_lba_sums, dim3(1), dim3(kLmLanes), V, 1, lambda);
    rc = fetch();
    *ok = h_rec->ok != 0; *chi = h_rec->chi; *scale = h_rec->scale;
    return rc == RGBL_OK;
  }
  bool accept() {
    hipError_t e = hipMemcpyAsync(V.T, V.Tt, sizeof(PoPose) * (size_t)V.nC, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(V.X, V.Xt, sizeof(double) * 3 * (size_t)V.nP, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); rc = RGBL_ERR_HIP; }
    return e == hipSuccess;
  }
};

}  // namespace rgbl_lba
