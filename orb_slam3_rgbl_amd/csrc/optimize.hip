// optimize.hip — the two Levenberg optimisers on the device, one workgroup per problem, and their host entry points:
//   k_pose_opt   Optimizer::PoseOptimization (src/Optimizer.cc:814-1114), csrc/poseopt_math.h
//   k_sim3_opt   Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381), csrc/sim3opt_math.h
// with lm_tree_reduce, the workgroup's execution of csrc/lm_math.h's fixed summation tree, and the device test hooks of the
// two headers (k_test_po_math, k_test_so_exp).  A call is staged through csrc/matcher_call.h.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "common.h"
#include "matcher_call.h"
#include "poseopt_math.h"
#include "sim3opt_math.h"

namespace rgbl {

// ------------------------------------------------------------------------------------------------
// Optimizer::PoseOptimization (src/Optimizer.cc:814-1114): k_pose_opt, one workgroup of 256 work-items per problem.  The
// algorithm is po_optimize of csrc/poseopt_math.h, run by every work-item: the scalar state (pose, lambda, the 6 x 6 solve,
// the update) is computed redundantly and identically, the edges are spread over the lanes (edge k on lane k mod 256).  No
// communication between workgroups, no atomics; the barriers of lm_tree_reduce are the only synchronisation and every
// work-item reaches every one of them (all branches around them depend on reduced values only).  Every loop is bounded by
// 4 rounds x 10 iterations x 10 trials.
struct PoseOptProblem {
  const float* xy;       // the frame's mvKeysUn (resident or staged)
  const int32_t* oct;
  const float* ur;
  const float* wpos;     // world positions: the call's staged array or the pool's
  const float* sigma;    // mvInvLevelSigma2
  int edge_off, m, n_levels;
  float q[4], t[3], K[4], bf;
};
struct PoseOptDev {
  const PoseOptProblem* prob;
  const int32_t* feat;   // per correspondence (all problems back to back): the feature ...
  const int32_t* point;  // ... and its row of wpos
  double* chi2;          // the state of the edges beyond 8 per lane
  uint8_t* level;        // every edge's level: the result, and the state of the edges beyond 8 per lane (starts 0)
  float* pose;           // 8 floats per problem: q, t
  int32_t* ret;
  PoDiag* diag;
};

__device__ __forceinline__ PoEdge pose_opt_edge(const PoseOptProblem& pb, const PoseOptDev& D, int k) {
  const int f = D.feat[pb.edge_off + k], p = D.point[pb.edge_off + k];
  PoEdge e;
  e.Xw[0] = pb.wpos[3 * (size_t)p]; e.Xw[1] = pb.wpos[3 * (size_t)p + 1]; e.Xw[2] = pb.wpos[3 * (size_t)p + 2];
  e.obs[0] = pb.xy[2 * f]; e.obs[1] = pb.xy[2 * f + 1]; e.obs[2] = pb.ur[f];
  const int oc = pb.oct[f], o = oc < 0 ? 0 : (oc >= pb.n_levels ? pb.n_levels - 1 : oc);   // host arrays are checked before the launch
  e.info = pb.sigma[o];
  e.stereo = e.obs[2] >= 0.0f ? 1 : 0;   // !(mvuRight[i] < 0) (:866)
  e.level = 0;
  e.chi2 = 0.0;
  return e;
}

// The workgroup's execution of csrc/lm_math.h's fixed tree v[i] = v[i] + v[i + s] over the first N sums of every lane's acc:
// lanes 64 .. 255 put their sums into LDS and wave 0 forms (v[i] + v[i + 128]) + (v[i + 64] + v[i + 192]), which is what s = 128
// and s = 64 leave in lane i < 64; s = 32 .. 1 run inside wave 0 (lane i reads lane i + s; lanes >= s compute values nobody
// reads), all sums side by side so that the cross-lane reads overlap; lane 0 writes the result to dst (LDS), where every
// work-item reads it.  Two barriers.
constexpr int kLmTreeLds = kLmLanes - 64;   // the partial sums of lanes 64 .. 255
template <int N> __device__ __forceinline__ void lm_tree_reduce(const double* acc, double (*red)[kLmTreeLds], double* dst, int tid) {
  if (tid >= 64) {
#pragma unroll
    for (int c = 0; c < N; ++c) red[c][tid - 64] = acc[c];
  }
  __syncthreads();
  if (tid < 64) {
    double v[N];
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = (acc[c] + red[c][tid + 64]) + (red[c][tid] + red[c][tid + 128]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int c = 0; c < N; ++c) v[c] = v[c] + __shfl_down(v[c], (unsigned)s);
    }
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < N; ++c) dst[c] = v[c];
    }
  }
  __syncthreads();
}

struct PoDevLanes {
  PoEdge r[kPoRegEdges];   // edges tid, tid + 256, ... in registers
  double acc[kPoSums];
  const PoseOptProblem* pb;
  const PoseOptDev* D;
  double (*red)[kLmTreeLds];
  double* bc;
  int tid, m;
  __device__ void zero() {
#pragma unroll
    for (int c = 0; c < kPoSums; ++c) acc[c] = 0.0;
  }
  template <class F> __device__ void each(F f) {
#pragma unroll
    for (int j = 0; j < kPoRegEdges; ++j)
      if (tid + kPoLanes * j < m) f(r[j], acc);
    for (int k = tid + kPoLanes * kPoRegEdges; k < m; k += kPoLanes) {   // beyond 2048 correspondences: global memory
      PoEdge e = pose_opt_edge(*pb, *D, k);
      e.chi2 = D->chi2[pb->edge_off + k];
      e.level = D->level[pb->edge_off + k];
      f(e, acc);
      D->chi2[pb->edge_off + k] = e.chi2;
      D->level[pb->edge_off + k] = e.level;
    }
  }
  // every work-item copies the system's 28 sums from bc to registers (the trials' solves read them there: measured against
  // reading them from LDS, docs/history/r15_measured.md), so the single sum can go through bc[0]
  __device__ const double* reduce_system(double* S) {
    lm_tree_reduce<kPoSums>(acc, red, bc, tid);
#pragma unroll
    for (int c = 0; c < kPoSums; ++c) S[c] = bc[c];
    return S;
  }
  __device__ double reduce_one() { lm_tree_reduce<1>(acc, red, bc, tid); return bc[0]; }
};

__global__ __launch_bounds__(kPoLanes) void k_pose_opt(PoseOptDev D) {
  __shared__ double s_red[kPoSums][kLmTreeLds];   // 42 KB
  __shared__ double s_bc[kPoSums];
  const PoseOptProblem& pb = D.prob[blockIdx.x];
  PoDevLanes G;
  G.pb = &pb; G.D = &D; G.red = s_red; G.bc = s_bc; G.tid = (int)threadIdx.x; G.m = pb.m;
#pragma unroll
  for (int j = 0; j < kPoRegEdges; ++j) {
    const int k = G.tid + kPoLanes * j;
    if (k < pb.m) G.r[j] = pose_opt_edge(pb, D, k);
  }
  const PoCam C = {(double)pb.K[0], (double)pb.K[1], (double)pb.K[2], (double)pb.K[3], (double)pb.bf};
  const PoPose entry = po_pose_from_float(pb.q, pb.t);
  PoPose out;
  PoDiag diag;
  const int ret = po_optimize(G, C, entry, pb.m, out, diag);
#pragma unroll
  for (int j = 0; j < kPoRegEdges; ++j) {
    const int k = G.tid + kPoLanes * j;
    if (k < pb.m) D.level[pb.edge_off + k] = G.r[j].level;
  }
  if (threadIdx.x == 0) {
    float* o = D.pose + 8 * (size_t)blockIdx.x;
    for (int i = 0; i < 4; ++i) o[i] = (float)out.q[i];
    for (int i = 0; i < 3; ++i) o[4 + i] = (float)out.t[i];
    o[7] = 0.0f;
    D.ret[blockIdx.x] = ret;
    D.diag[blockIdx.x] = diag;
  }
}

// test hook: the header's sin / cos and the fp64 quotient and square root on the device (op 0: sin, 1: cos, 2: x / y, 3: sqrt)
__global__ void k_test_po_math(int op, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ z, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  z[i] = op == 0 ? po_sin(x[i]) : op == 1 ? po_cos(x[i]) : op == 2 ? x[i] / y[i] : sqrt(x[i]);
}

// ------------------------------------------------------------------------------------------------
// Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381): k_sim3_opt, one workgroup of 256 work-items per problem, after
// k_pose_opt.  The algorithm is so_optimize of csrc/sim3opt_math.h, run by every work-item: the scalar state (estimate, lambda,
// the 7 x 7 solve, the update) is computed redundantly and identically, the edge pairs are spread over the lanes (pair k on
// lane k mod 256).  The host hands over the CANDIDATES (the features that pass :2169-2233); the workgroup forms P3D2c, applies
// the float test of :2235 and numbers the survivors in ascending feature index with a ballot scan, 256 candidates at a time
// (at most 256 chunks).  The 30 transforms of a linearisation are computed by work-items 0 .. 14 and kept in LDS.  No
// communication between workgroups, no atomics; every work-item reaches every barrier (all branches around them depend on
// reduced values only).  The optimiser's loops are bounded by (5 + 10) iterations x 10 trials.
struct Sim3OptProblem {
  const float *xy1, *xy2;        // mvKeysUn of both key frames (resident or staged)
  const int32_t *oct1, *oct2;
  const float* wpos;             // world positions: the call's staged array or the pool's
  const float *sig1, *sig2;      // mvInvLevelSigma2 of both
  int cand_off, n_cand, n_levels1, n_levels2, fix_scale;
  float th2;
  float Rcw1[9], tcw1[3], Rcw2[9], tcw2[3], K1[4], K2[4];
  SoSim3 entry;
  SoDiag diag;                   // the host's counters (n_bad_mps, n_without_mp); the others are the kernel's
};
struct Sim3OptOut {
  SoSim3 est;
  SoDiag diag;
  int32_t ret, reserved;
};
struct Sim3OptDev {
  const Sim3OptProblem* prob;
  const int32_t *feat, *p1, *p2, *i2, *lvl2;   // per candidate (all problems back to back): feature, rows of wpos, i2, mnTrackScaleLevel
  int32_t* corr;       // per correspondence k of a problem (at cand_off + k): its candidate
  double* chi;         // the state of the pairs beyond 8 per lane: chi12, chi21 ...
  uint8_t* state;      // ... and gone | cleared << 1
  uint8_t* cleared;    // per candidate: the result (2: no edge pair)
  Sim3OptOut* out;
};

__device__ __forceinline__ int clamp_level(int o, int n_levels) { return o < 0 ? 0 : (o >= n_levels ? n_levels - 1 : o); }   // host arrays are checked before the launch

__device__ __forceinline__ bool sim3_opt_edge(const Sim3OptProblem& pb, const Sim3OptDev& D, int c, SoEdge& e) {
  const int g = pb.cand_off + c, f = D.feat[g], i2 = D.i2[g];
  const float info1 = pb.sig1[clamp_level(pb.oct1[f], pb.n_levels1)];
  const float info2 = pb.sig2[clamp_level(i2 >= 0 ? pb.oct2[i2] : D.lvl2[g], pb.n_levels2)];
  return so_make_edge(pb.Rcw1, pb.tcw1, pb.Rcw2, pb.tcw2, pb.wpos + 3 * (size_t)D.p1[g], pb.wpos + 3 * (size_t)D.p2[g], pb.xy1 + 2 * (size_t)f,
                      info1, i2 >= 0, pb.xy2 + 2 * (size_t)(i2 >= 0 ? i2 : 0), info2, e);
}

// A pair's twelve floats are used as doubles in every pass over the edges.  Left alone, the compiler converts them once and
// keeps the doubles for the whole kernel: 24 more registers per pair.  An empty statement the value passes through makes the
// conversion belong to the pass.
#ifdef RGBL_EMU
#define SO_OPAQUE(x) ((void)0)
#else
#define SO_OPAQUE(x) asm volatile("" : "+v"(x))
#endif
struct SoDevLanes {
  SoEdge r[kSoRegEdges];   // pairs tid, tid + 256, ... in registers
  double acc[kSoSums];
  const Sim3OptProblem* pb;
  const Sim3OptDev* D;
  double (*red)[kLmTreeLds];
  double* bc;
  SoSim3* T;
  int tid, m;
  __device__ void zero() {
#pragma unroll
    for (int c = 0; c < kSoSums; ++c) acc[c] = 0.0;
  }
  template <class F> __device__ void each(F f) {
#pragma unroll
    for (int j = 0; j < kSoRegEdges; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { SO_OPAQUE(r[j].X1[c]); SO_OPAQUE(r[j].X2[c]); }
      SO_OPAQUE(r[j].obs1[0]); SO_OPAQUE(r[j].obs1[1]); SO_OPAQUE(r[j].obs2[0]); SO_OPAQUE(r[j].obs2[1]);
      SO_OPAQUE(r[j].info1); SO_OPAQUE(r[j].info2);
      if (tid + kSoLanes * j < m) f(r[j], acc);
    }
    for (int k = tid + kSoLanes * kSoRegEdges; k < m; k += kSoLanes) {   // beyond 2048 correspondences: global memory
      const size_t g = (size_t)pb->cand_off + (size_t)k;
      SoEdge e;
      sim3_opt_edge(*pb, *D, D->corr[g], e);
      e.chi12 = D->chi[2 * g]; e.chi21 = D->chi[2 * g + 1];
      e.gone = D->state[g] & 1; e.cleared = D->state[g] >> 1;
      f(e, acc);
      D->chi[2 * g] = e.chi12; D->chi[2 * g + 1] = e.chi21;
      D->state[g] = (uint8_t)(e.gone | (e.cleared << 1));
    }
  }
  // the system's 36 sums stay in bc[0 .. 35] for the trials' solves; the single sum goes through bc[36]
  __device__ const double* reduce_system(double*) { lm_tree_reduce<kSoSums>(acc, red, bc, tid); return bc; }
  __device__ double reduce_one() { lm_tree_reduce<1>(acc, red, bc + kSoSums, tid); return bc[kSoSums]; }
  // work-item j < 14 forms perturbed estimate j and its inverse, work-item 14 the estimate's inverse; the readers of the
  // previous linearisation are behind the barriers of the reductions in between
  __device__ const SoSim3* transforms(const SoSim3& S, bool fix_scale) {
    if (tid < 14) {
      const SoSim3 P = so_perturbed(S, tid, fix_scale);
      T[2 + tid] = P;
      T[16 + tid] = so_inverse(P);
    } else if (tid == 14) {
      T[0] = S;
      T[1] = so_inverse(S);
    }
    __syncthreads();
    return T;
  }
};

__global__ __launch_bounds__(kSoLanes) void k_sim3_opt(Sim3OptDev D) {
  __shared__ double s_red[kSoSums][kLmTreeLds];   // 54 KB
  __shared__ double s_bc[kSoSums + 1];
  __shared__ SoSim3 s_T[kSoTransforms];           // 1920 B
  __shared__ int s_cnt[4][2];
  const Sim3OptProblem& pb = D.prob[blockIdx.x];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // :2235 and the numbering of the correspondences
  int m = 0, n_in = 0;
  for (int c0 = 0; c0 < pb.n_cand; c0 += kSoLanes) {   // uniform
    const int c = c0 + tid;
    bool keep = false, in2 = false;
    if (c < pb.n_cand) {
      float X2[3];
      s3_transform(pb.Rcw2, pb.tcw2, pb.wpos + 3 * (size_t)D.p2[pb.cand_off + c], X2);
      keep = !(X2[2] < 0.0f);
      in2 = keep && D.i2[pb.cand_off + c] >= 0;
    }
    const unsigned long long bk = __ballot(keep), bi = __ballot(in2);
    if (lane == 0) { s_cnt[wave][0] = __popcll(bk); s_cnt[wave][1] = __popcll(bi); }
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += s_cnt[w][0];
      total += s_cnt[w][0];
      n_in += s_cnt[w][1];
    }
    if (keep) D.corr[pb.cand_off + m + before + __popcll(bk & ((1ull << lane) - 1ull))] = c;   // < cand_off + n_cand
    m += total;
    __syncthreads();
  }
  SoDevLanes G;
  G.pb = &pb; G.D = &D; G.red = s_red; G.bc = s_bc; G.T = s_T; G.tid = tid; G.m = m;
#pragma unroll
  for (int j = 0; j < kSoRegEdges; ++j) {
    const int k = tid + kSoLanes * j;
    if (k < m) sim3_opt_edge(pb, D, D.corr[pb.cand_off + k], G.r[j]);
  }
  for (int k = tid + kSoLanes * kSoRegEdges; k < m; k += kSoLanes) D.state[pb.cand_off + k] = 0;
  const SoCam C1 = {(double)pb.K1[0], (double)pb.K1[1], (double)pb.K1[2], (double)pb.K1[3]};
  const SoCam C2 = {(double)pb.K2[0], (double)pb.K2[1], (double)pb.K2[2], (double)pb.K2[3]};
  SoSim3 est;
  SoDiag diag = pb.diag;
  diag.n_correspondences = m; diag.n_in_kf2 = n_in; diag.n_out_kf2 = m - n_in;
  const int ret = so_optimize(G, C1, C2, pb.entry, m, pb.th2, pb.fix_scale != 0, est, diag);
#pragma unroll
  for (int j = 0; j < kSoRegEdges; ++j) {
    const int k = tid + kSoLanes * j;
    if (k < m) D.cleared[pb.cand_off + D.corr[pb.cand_off + k]] = G.r[j].cleared;
  }
  for (int k = tid + kSoLanes * kSoRegEdges; k < m; k += kSoLanes)
    D.cleared[pb.cand_off + D.corr[pb.cand_off + k]] = D.state[pb.cand_off + k] >> 1;
  if (tid == 0) {
    Sim3OptOut& o = D.out[blockIdx.x];
    o.est = est;
    o.diag = diag;
    o.ret = ret;
    o.reserved = 0;
  }
}

// test hook: the header's exp on the device
__global__ void k_test_so_exp(const double* __restrict__ x, double* __restrict__ z, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[i] = so_exp(x[i]);
}

}  // namespace rgbl

using namespace rgbl;

extern "C" {

// ---- Optimizer::PoseOptimization (src/Optimizer.cc:814-1114) ---------------------------------------------------------
namespace {
// everything that can be refused is refused here, before anything is staged, launched or written; counts the correspondences
int check_pose_opt_input(const rgbl_pose_opt_input* in, int b, bool host_only, int* n_corr) {
  *n_corr = 0;
  if (in->n < 0 || in->n > 65535 || in->n_points < 0 || (in->n > 0 && !in->mp_index)) { set_error("pose optimisation %d: n outside [0, 65535], n_points < 0 or no mp_index", b); return RGBL_ERR_INVALID; }
  if (in->n_levels < 1 || in->n_levels > kProjMaxLevels || !in->inv_level_sigma2) { set_error("pose optimisation %d: n_levels outside [1, %d] or no inv_level_sigma2", b, kProjMaxLevels); return RGBL_ERR_INVALID; }
  bool finite = std::isfinite(in->bf);
  for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->Tcw_q[i]) && std::isfinite(in->K[i]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(in->Tcw_t[i]);
  if (!finite) { set_error("pose optimisation %d: the pose, K or bf is not finite", b); return RGBL_ERR_INVALID; }
  if (host_only && (in->device || in->pool)) { set_error("pose optimisation %d: the host build reads host arrays only", b); return RGBL_ERR_INVALID; }
  if (in->device ? in->device->n != in->n : (in->n > 0 && (!in->kp_xy || !in->kp_octave || !in->uright))) {
    set_error("pose optimisation %d: the frame side is either kp_xy, kp_octave, uright or a resident frame of n features", b);
    return RGBL_ERR_INVALID;
  }
  if (in->n_points > 0 && (in->pool ? !in->slot : !in->world_pos)) { set_error("pose optimisation %d: the map side is either world_pos or a pool with slot", b); return RGBL_ERR_INVALID; }
  return check_correspondences("pose optimisation", b, in->n, in->mp_index, in->n_points, in->device ? nullptr : in->kp_octave, in->n_levels, n_corr);
}
// what :869 / :897 and :1107-1113 leave in the caller's arrays, from the level of every correspondence
void write_pose_opt_output(const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out, const float pose[7], const uint8_t* level, int ret,
                           const PoDiag& diag) {
  const bool untouched = diag.rounds == 0;   // fewer than 3 correspondences: the pose is not written (:996-997)
  memcpy(out->Tcw_q, untouched ? in->Tcw_q : pose, sizeof(out->Tcw_q));
  memcpy(out->Tcw_t, untouched ? in->Tcw_t : pose + 4, sizeof(out->Tcw_t));
  if (out->outlier) {
    int k = 0;
    for (int i = 0; i < in->n; ++i)
      if (in->mp_index[i] >= 0) out->outlier[i] = level[k++];
  }
  out->result = ret;
  static_assert(sizeof(PoDiag) == sizeof(rgbl_pose_opt_diag), "PoDiag is rgbl_pose_opt_diag");
  memcpy(&out->diag, &diag, sizeof(diag));
}
}  // namespace

int rgbl_pose_optimization_host(const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  int m = 0;
  RGBL_TRY(check_pose_opt_input(in, 0, true, &m));
  std::vector<PoEdge> edges((size_t)m);
  int k = 0;
  for (int i = 0; i < in->n; ++i) {
    const int p = in->mp_index[i];
    if (p < 0) continue;
    PoEdge& e = edges[(size_t)k++];
    for (int c = 0; c < 3; ++c) e.Xw[c] = in->world_pos[3 * (size_t)p + c];
    e.obs[0] = in->kp_xy[2 * i]; e.obs[1] = in->kp_xy[2 * i + 1]; e.obs[2] = in->uright[i];
    e.info = in->inv_level_sigma2[in->kp_octave[i]];
    e.stereo = e.obs[2] >= 0.0f ? 1 : 0;
    e.level = 0;
    e.chi2 = 0.0;
  }
  std::vector<LmHostLanes<PoEdge, kPoSums>> lanes(1, LmHostLanes<PoEdge, kPoSums>(edges.data(), m));   // 57 KB: not on the stack
  const PoCam C = {(double)in->K[0], (double)in->K[1], (double)in->K[2], (double)in->K[3], (double)in->bf};
  PoPose T;
  PoDiag diag;
  const int ret = po_optimize(lanes[0], C, po_pose_from_float(in->Tcw_q, in->Tcw_t), m, T, diag);
  float pose[7];
  for (int i = 0; i < 4; ++i) pose[i] = (float)T.q[i];
  for (int i = 0; i < 3; ++i) pose[4 + i] = (float)T.t[i];
  std::vector<uint8_t> level((size_t)m);
  for (int i = 0; i < m; ++i) level[(size_t)i] = edges[(size_t)i].level;
  write_pose_opt_output(in, out, pose, level.data(), ret, diag);
  return RGBL_OK;
}

int rgbl_pose_optimization_batch(rgbl_matcher* m, int n_problems, const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out) {
  if (!m || n_problems < 0 || (n_problems > 0 && (!in || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int B = n_problems;
  std::vector<int> off((size_t)B + 1, 0);
  PoolCall pc(m, "pose optimisation", "the frame");
  for (int b = 0; b < B; ++b) {
    int mb = 0;
    RGBL_TRY(check_pose_opt_input(in + b, b, false, &mb));
    if (off[(size_t)b] > INT_MAX - mb) { set_error("pose optimisation: more than 2^31 correspondences in one call"); return RGBL_ERR_INVALID; }
    off[(size_t)b + 1] = off[(size_t)b] + mb;
    RGBL_TRY(pc.note(in[b].pool, {in[b].device}, b));
  }
  if (B == 0) return RGBL_OK;
  const int M = off[(size_t)B];
  const rgbl_map_points* pool = pc.pool;
  RGBL_TRY(pc.lock(B, [&](int b) -> int {
    for (int i = 0; in[b].pool && i < in[b].n_points; ++i)
      if (!pc.holds(in[b].slot[i])) { set_error("pose optimisation %d: slot %d outside [0, %d)", b, in[b].slot[i], pool->cap); return RGBL_ERR_INVALID; }
    return RGBL_OK;
  }));
  // the correspondences of all problems back to back: feature, and row of the problem's world positions
  std::vector<int32_t> feat((size_t)M), point((size_t)M);
  for (int b = 0; b < B; ++b)
    list_correspondences(in[b].n, in[b].mp_index, in[b].pool ? in[b].slot : nullptr, feat.data() + off[(size_t)b], point.data() + off[(size_t)b]);
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // behind pc (PoolCall)
  HostCall hc(m);
  hipStream_t s = hc.s;
  std::vector<PoseOptProblem> prob((size_t)B);
  PoseOptDev D;
  memset(&D, 0, sizeof(D));
  RGBL_TRY(hc.begin([&]() -> int {
    for (int b = 0; b < B; ++b) {
      PoseOptProblem& P = prob[(size_t)b];
      memset(&P, 0, sizeof(P));
      const rgbl_pose_opt_input& I = in[b];
      RGBL_TRY(put_features(hc, I.device, I.n, nullptr, I.kp_xy, I.kp_octave, I.uright, nullptr, &P.xy, &P.oct, &P.ur));
      if (I.pool) P.wpos = pool->d_wpos; else hc.put(&P.wpos, I.world_pos, (size_t)I.n_points * 3);
      hc.put(&P.sigma, I.inv_level_sigma2, (size_t)I.n_levels);
      P.edge_off = off[(size_t)b]; P.m = off[(size_t)b + 1] - off[(size_t)b]; P.n_levels = I.n_levels;
      memcpy(P.q, I.Tcw_q, sizeof(P.q)); memcpy(P.t, I.Tcw_t, sizeof(P.t)); memcpy(P.K, I.K, sizeof(P.K));
      P.bf = I.bf;
    }
    hc.put(&D.feat, feat.data(), (size_t)M);
    hc.put(&D.point, point.data(), (size_t)M);
    D.prob = hc.stage<PoseOptProblem>((size_t)B, [&](PoseOptProblem* dst) { memcpy(dst, prob.data(), sizeof(PoseOptProblem) * (size_t)B); });
    D.level = hc.put_fill<uint8_t>((size_t)M, 0);   // what comes back, side by side
    hc.mark_result(D.level, (size_t)M);
    D.pose = hc.result<float>((size_t)B * 8);
    D.ret = hc.result<int32_t>((size_t)B);
    D.diag = hc.result<PoDiag>((size_t)B);
    D.chi2 = hc.scratch<double>((size_t)M);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_pose_opt", k_pose_opt, dim3((unsigned)B), dim3(kPoLanes), 0, D));
  RGBL_TRY(hc.fetch());
  for (int b = 0; b < B; ++b)
    write_pose_opt_output(in + b, out + b, hc.host(D.pose) + 8 * (size_t)b, hc.host(D.level) + off[(size_t)b], hc.host(D.ret)[b], hc.host(D.diag)[b]);
  return RGBL_OK;
}

int rgbl_pose_optimization(rgbl_matcher* m, const rgbl_pose_opt_input* in, rgbl_pose_opt_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return rgbl_pose_optimization_batch(m, 1, in, out);
}

// ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) --------------------------------------------------------------
namespace {
struct Sim3OptCand { int32_t feat, p1, p2, i2, lvl2; };
// Everything that can be refused without the pool is refused here, before anything is staged, launched or written.  Runs
// :2167-2233: counts nBadMPs and nMatchWithoutMP and lists the candidates, the features that reach the depth test of :2235.
int check_sim3_opt_input(const rgbl_sim3_opt_input* in, int b, bool host_only, std::vector<Sim3OptCand>* cand, SoDiag* diag) {
  memset(diag, 0, sizeof(*diag));
  if (in->n < 0 || in->n > 65535 || in->n2 < 0 || in->n2 > 65535 || in->n_points < 0) { set_error("sim3 optimisation %d: n or n2 outside [0, 65535], or n_points < 0", b); return RGBL_ERR_INVALID; }
  if (in->n > 0 && (!in->mp1_index || !in->match_index || !in->i2 || !in->track_level2)) { set_error("sim3 optimisation %d: no mp1_index, match_index, i2 or track_level2", b); return RGBL_ERR_INVALID; }
  if (in->n_levels1 < 1 || in->n_levels1 > kProjMaxLevels || in->n_levels2 < 1 || in->n_levels2 > kProjMaxLevels || !in->inv_level_sigma2_1 || !in->inv_level_sigma2_2) {
    set_error("sim3 optimisation %d: n_levels outside [1, %d] or no inv_level_sigma2", b, kProjMaxLevels);
    return RGBL_ERR_INVALID;
  }
  bool finite = std::isfinite(in->th2) && std::isfinite(in->s);
  for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->K1[i]) && std::isfinite(in->K2[i]) && std::isfinite(in->q[i]);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(in->Rcw1[i]) && std::isfinite(in->Rcw2[i]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(in->tcw1[i]) && std::isfinite(in->tcw2[i]) && std::isfinite(in->t[i]);
  if (!finite) { set_error("sim3 optimisation %d: a pose, K, th2 or the estimate is not finite", b); return RGBL_ERR_INVALID; }
  if (host_only && (in->device1 || in->device2 || in->pool)) { set_error("sim3 optimisation %d: the host build reads host arrays only", b); return RGBL_ERR_INVALID; }
  if (in->device1 ? in->device1->n != in->n : (in->n > 0 && (!in->kp1_xy || !in->kp1_octave))) {
    set_error("sim3 optimisation %d: key frame 1 is either kp1_xy, kp1_octave or a resident frame of n features", b);
    return RGBL_ERR_INVALID;
  }
  if (in->device2 ? in->device2->n != in->n2 : (in->n2 > 0 && (!in->kp2_xy || !in->kp2_octave))) {
    set_error("sim3 optimisation %d: key frame 2 is either kp2_xy, kp2_octave or a resident frame of n2 features", b);
    return RGBL_ERR_INVALID;
  }
  if (in->n_points > 0 && (!in->bad || (in->pool ? !in->slot : !in->world_pos))) { set_error("sim3 optimisation %d: no bad flags, or the map side is neither world_pos nor a pool with slot", b); return RGBL_ERR_INVALID; }
  for (int i = 0; i < in->n; ++i) {
    const int p1 = in->mp1_index[i], p2 = in->match_index[i];
    if (p1 < -1 || p1 >= in->n_points || p2 < -1 || p2 >= in->n_points) { set_error("sim3 optimisation %d: mp1_index / match_index of feature %d = (%d, %d) outside [-1, %d)", b, i, p1, p2, in->n_points); return RGBL_ERR_INVALID; }
    if (p2 < 0) continue;                                                 // :2169
    const int i2 = in->i2[i];
    if (i2 < -1 || i2 >= in->n2) { set_error("sim3 optimisation %d: i2 of feature %d = %d outside [-1, %d)", b, i, i2, in->n2); return RGBL_ERR_INVALID; }
    if (p1 < 0) { ++diag->n_without_mp; continue; }                       // :2209-2227
    if (in->bad[p1] || in->bad[p2]) { ++diag->n_bad_mps; continue; }      // :2203-2207
    if (i2 < 0 && !in->all_points) continue;                              // :2229
    // the levels are checked on every pair that reaches the depth test
    if (!in->device1 && (in->kp1_octave[i] < 0 || in->kp1_octave[i] >= in->n_levels1)) { set_error("sim3 optimisation %d: octave %d of feature %d outside [0, %d)", b, in->kp1_octave[i], i, in->n_levels1); return RGBL_ERR_INVALID; }
    if (i2 < 0 ? (in->track_level2[i] < 0 || in->track_level2[i] >= in->n_levels2)
               : (!in->device2 && (in->kp2_octave[i2] < 0 || in->kp2_octave[i2] >= in->n_levels2))) {
      set_error("sim3 optimisation %d: the level of feature %d's match outside [0, %d)", b, i, in->n_levels2);
      return RGBL_ERR_INVALID;
    }
    cand->push_back(Sim3OptCand{i, p1, p2, i2, in->track_level2[i]});
  }
  return RGBL_OK;
}
inline SoSim3 sim3_opt_entry(const rgbl_sim3_opt_input* in) {
  SoSim3 S;
  memcpy(S.q, in->q, sizeof(S.q)); memcpy(S.t, in->t, sizeof(S.t));
  S.s = in->s;
  return S;
}
// `flag` per candidate: 0 / 1 the pair's cleared flag, 2 no pair
void write_sim3_opt_output(const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out, const Sim3OptCand* cand, int n_cand, const uint8_t* flag,
                           const SoSim3& est, int ret, const SoDiag& diag) {
  out->result = ret;
  memcpy(out->q, est.q, sizeof(out->q)); memcpy(out->t, est.t, sizeof(out->t));
  out->s = est.s;
  if (out->cleared)
    for (int c = 0; c < n_cand; ++c)
      if (flag[c] != 2) out->cleared[cand[c].feat] = flag[c];
  static_assert(sizeof(SoDiag) == sizeof(rgbl_sim3_opt_diag), "SoDiag is rgbl_sim3_opt_diag");
  memcpy(&out->diag, &diag, sizeof(diag));
}
}  // namespace

int rgbl_optimize_sim3_host(const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  std::vector<Sim3OptCand> cand;
  SoDiag diag;
  RGBL_TRY(check_sim3_opt_input(in, 0, true, &cand, &diag));
  const int nc = (int)cand.size();
  std::vector<SoEdge> edges;
  std::vector<int> edge_cand;
  for (int c = 0; c < nc; ++c) {
    const Sim3OptCand& k = cand[(size_t)c];
    SoEdge e;
    const float info1 = in->inv_level_sigma2_1[in->kp1_octave[k.feat]];
    const float info2 = in->inv_level_sigma2_2[k.i2 >= 0 ? in->kp2_octave[k.i2] : k.lvl2];
    if (!so_make_edge(in->Rcw1, in->tcw1, in->Rcw2, in->tcw2, in->world_pos + 3 * (size_t)k.p1, in->world_pos + 3 * (size_t)k.p2,
                      in->kp1_xy + 2 * (size_t)k.feat, info1, k.i2 >= 0, k.i2 >= 0 ? in->kp2_xy + 2 * (size_t)k.i2 : nullptr, info2, e))
      continue;
    edges.push_back(e);
    edge_cand.push_back(c);
    if (k.i2 >= 0) ++diag.n_in_kf2; else ++diag.n_out_kf2;
  }
  const int m = (int)edges.size();
  diag.n_correspondences = m;
  std::vector<SoHostLanes> lanes(1, SoHostLanes(edges.data(), m));   // 75 KB: not on the stack
  const SoCam C1 = {(double)in->K1[0], (double)in->K1[1], (double)in->K1[2], (double)in->K1[3]};
  const SoCam C2 = {(double)in->K2[0], (double)in->K2[1], (double)in->K2[2], (double)in->K2[3]};
  SoSim3 est;
  const int ret = so_optimize(lanes[0], C1, C2, sim3_opt_entry(in), m, in->th2, in->fix_scale != 0, est, diag);
  std::vector<uint8_t> flag((size_t)nc, 2);
  for (int k = 0; k < m; ++k) flag[(size_t)edge_cand[(size_t)k]] = edges[(size_t)k].cleared;
  write_sim3_opt_output(in, out, cand.data(), nc, flag.data(), est, ret, diag);
  return RGBL_OK;
}

int rgbl_optimize_sim3_batch(rgbl_matcher* m, int n_problems, const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out) {
  if (!m || n_problems < 0 || (n_problems > 0 && (!in || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int B = n_problems;
  if (B > 32767) { set_error("sim3 optimisation: more than 32767 problems in one call"); return RGBL_ERR_INVALID; }
  std::vector<int> off((size_t)B + 1, 0);   // at most 65535 candidates each: B < 2^15 problems fit an int
  std::vector<Sim3OptCand> cand;
  std::vector<SoDiag> diag((size_t)B);
  PoolCall pc(m, "sim3 optimisation", "a frame");
  for (int b = 0; b < B; ++b) {
    RGBL_TRY(check_sim3_opt_input(in + b, b, false, &cand, &diag[(size_t)b]));
    off[(size_t)b + 1] = (int)cand.size();
    RGBL_TRY(pc.note(in[b].pool, {in[b].device1, in[b].device2}, b));
  }
  if (B == 0) return RGBL_OK;
  const int M = off[(size_t)B];
  const rgbl_map_points* pool = pc.pool;
  RGBL_TRY(pc.lock(B, [&](int b) -> int {
    for (int i = 0; in[b].pool && i < in[b].n_points; ++i)
      if (!pc.holds(in[b].slot[i])) { set_error("sim3 optimisation %d: slot %d outside [0, %d)", b, in[b].slot[i], pool->cap); return RGBL_ERR_INVALID; }
    return RGBL_OK;
  }));
  // the candidates of all problems back to back
  std::vector<int32_t> feat((size_t)M), p1((size_t)M), p2((size_t)M), i2((size_t)M), lvl2((size_t)M);
  for (int b = 0; b < B; ++b)
    for (int c = off[(size_t)b]; c < off[(size_t)b + 1]; ++c) {
      const Sim3OptCand& k = cand[(size_t)c];
      feat[(size_t)c] = k.feat; i2[(size_t)c] = k.i2; lvl2[(size_t)c] = k.lvl2;
      p1[(size_t)c] = in[b].pool ? in[b].slot[k.p1] : k.p1;
      p2[(size_t)c] = in[b].pool ? in[b].slot[k.p2] : k.p2;
    }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // behind pc (PoolCall)
  HostCall hc(m);
  hipStream_t s = hc.s;
  std::vector<Sim3OptProblem> prob((size_t)B);
  Sim3OptDev D;
  memset(&D, 0, sizeof(D));
  RGBL_TRY(hc.begin([&]() -> int {
    for (int b = 0; b < B; ++b) {
      Sim3OptProblem& P = prob[(size_t)b];
      memset(&P, 0, sizeof(P));
      const rgbl_sim3_opt_input& I = in[b];
      RGBL_TRY(put_features(hc, I.device1, I.n, nullptr, I.kp1_xy, I.kp1_octave, nullptr, nullptr, &P.xy1, &P.oct1, nullptr));
      RGBL_TRY(put_features(hc, I.device2, I.n2, nullptr, I.kp2_xy, I.kp2_octave, nullptr, nullptr, &P.xy2, &P.oct2, nullptr));
      if (I.pool) P.wpos = pool->d_wpos; else hc.put(&P.wpos, I.world_pos, (size_t)I.n_points * 3);
      hc.put(&P.sig1, I.inv_level_sigma2_1, (size_t)I.n_levels1);
      hc.put(&P.sig2, I.inv_level_sigma2_2, (size_t)I.n_levels2);
      P.cand_off = off[(size_t)b]; P.n_cand = off[(size_t)b + 1] - off[(size_t)b];
      P.n_levels1 = I.n_levels1; P.n_levels2 = I.n_levels2; P.fix_scale = I.fix_scale ? 1 : 0; P.th2 = I.th2;
      memcpy(P.Rcw1, I.Rcw1, sizeof(P.Rcw1)); memcpy(P.tcw1, I.tcw1, sizeof(P.tcw1));
      memcpy(P.Rcw2, I.Rcw2, sizeof(P.Rcw2)); memcpy(P.tcw2, I.tcw2, sizeof(P.tcw2));
      memcpy(P.K1, I.K1, sizeof(P.K1)); memcpy(P.K2, I.K2, sizeof(P.K2));
      P.entry = sim3_opt_entry(&I);
      P.diag = diag[(size_t)b];
    }
    hc.put(&D.feat, feat.data(), (size_t)M);
    hc.put(&D.p1, p1.data(), (size_t)M);
    hc.put(&D.p2, p2.data(), (size_t)M);
    hc.put(&D.i2, i2.data(), (size_t)M);
    hc.put(&D.lvl2, lvl2.data(), (size_t)M);
    D.prob = hc.stage<Sim3OptProblem>((size_t)B, [&](Sim3OptProblem* dst) { memcpy(dst, prob.data(), sizeof(Sim3OptProblem) * (size_t)B); });
    D.cleared = hc.put_fill<uint8_t>((size_t)M, 2);   // what comes back, side by side
    hc.mark_result(D.cleared, (size_t)M);
    D.out = hc.result<Sim3OptOut>((size_t)B);
    D.corr = hc.scratch<int32_t>((size_t)M);
    D.chi = hc.scratch<double>((size_t)M * 2);
    D.state = hc.scratch<uint8_t>((size_t)M);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_sim3_opt", k_sim3_opt, dim3((unsigned)B), dim3(kSoLanes), 0, D));
  RGBL_TRY(hc.fetch());
  for (int b = 0; b < B; ++b) {
    const Sim3OptOut& o = hc.host(D.out)[b];
    write_sim3_opt_output(in + b, out + b, cand.data() + off[(size_t)b], off[(size_t)b + 1] - off[(size_t)b], hc.host(D.cleared) + off[(size_t)b], o.est, o.ret, o.diag);
  }
  return RGBL_OK;
}

int rgbl_optimize_sim3(rgbl_matcher* m, const rgbl_sim3_opt_input* in, rgbl_sim3_opt_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return rgbl_optimize_sim3_batch(m, 1, in, out);
}

// test hooks for csrc/sim3opt_math.h: so_exp on the host, and compiled for the device
double rgbl_test_so_exp(double x) { return so_exp(x); }
int rgbl_test_so_exp_device(const double* x, double* z, int n) {
  if (!x || !z || n < 1) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  return elementwise_device_hook<double>({x}, z, n, [&](double* const* d, double* dz, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_test_so_exp, grid, block, 0, 0, (const double*)d[0], dz, n);
  });
}

// test hooks for csrc/poseopt_math.h: op 0 sin, 1 cos, 2 x / y, 3 sqrt - on the host, and compiled for the device
double rgbl_test_po_math(int op, double x, double y) { return op == 0 ? po_sin(x) : op == 1 ? po_cos(x) : op == 2 ? x / y : sqrt(x); }
int rgbl_test_po_math_device(int op, const double* x, const double* y, double* z, int n) {
  if (!x || !y || !z || n < 1 || op < 0 || op > 3) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  return elementwise_device_hook<double>({x, y}, z, n, [&](double* const* d, double* dz, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_test_po_math, grid, block, 0, 0, op, (const double*)d[0], (const double*)d[1], dz, n);
  });
}

}  // extern "C"
