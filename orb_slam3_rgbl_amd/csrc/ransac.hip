// ransac.hip — the hypothesis-and-score solvers on the device, every hypothesis of a call at once, and their host entry points:
//   k_sim3_*    Sim3Solver (src/Sim3Solver.cc), csrc/sim3_math.h
//   k_mlpnp_*   MLPnPsolver (src/MLPnPsolver.cpp), csrc/mlpnp_math.h
//   k_tv_*      TwoViewReconstruction (src/TwoViewReconstruction.cc), csrc/twoview_math.h
// One wave per hypothesis; an inlier mask is 64-bit ballot words, a count their population count.  A call is staged through
// csrc/matcher_call.h.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "matcher_call.h"
#include "sim3_math.h"
#include "mlpnp_math.h"
#include "twoview_math.h"

namespace rgbl {

// bit i of a mask of 64-bit words
__host__ __device__ __forceinline__ unsigned long long mask_bit(const unsigned long long* words, int i) { return (words[i >> 6] >> (i & 63)) & 1ull; }

// One chunk of a hypothesis's inlier walk, run by one wave (lane l holds item 64 c + l's verdict): the ballot is word c of the
// hypothesis's bit mask, stored by lane 0, and its population count the chunk's inliers, the same in every lane.
__device__ __forceinline__ int wave_mask_word(bool in, int lane, unsigned long long* word) {
  const unsigned long long w = __ballot(in);
  if (lane == 0) *word = w;
  return __popcll(w);
}

// ------------------------------------------------------------------------------------------------
// Sim3Solver (src/Sim3Solver.cc): every hypothesis of a call at once.  The arithmetic is csrc/sim3_math.h.
//   k_sim3_hypotheses  grid (groups of 4 hypotheses, problem), 256 work-items: one wave per hypothesis.  The workgroup stages
//                      the problem's correspondences once in LDS (12 floats each: X1c, X2c, both own-image projections, both
//                      thresholds; problems beyond kS3LdsPoints read global memory and recompute them).  The closed form is
//                      wave-uniform: every lane computes it, no broadcast, no divergent branch.  A lane then takes every 64th
//                      correspondence; a chunk's count is a ballot and a population count, the ballot word is the chunk's
//                      part of the hypothesis's bit mask.  No atomics, no floating-point reduction.
//   k_sim3_select      one workgroup per problem: wave 0 runs the selection scan 64 hypotheses at a time (a prefix maximum and
//                      two ballots per chunk), then all work-items expand the selected mask into bytes.
// Both run on the call's stream, one behind the other; no workgroup waits for another.
constexpr int kS3LdsPoints = 1024;   // 48 KB of LDS
constexpr int kS3HypPerGroup = 4;
struct Sim3Problem {
  const float *x1, *x2;            // form 1: the staged camera-frame points
  const float* wpos;               // form 2: the pool's positions ...
  const int32_t *slot1, *slot2;    // ... and the slots
  const float *e1, *e2;            // the thresholds
  const int32_t* samples;
  int n, n_hyp;                    // n_hyp = 0: the problem is not run
  int hyp_off, word_off, words, inl_off;
  int fix_scale, min_inliers, best_inliers, pool_form;
  float K1[4], K2[4], Rcw1[9], tcw1[3], Rcw2[9], tcw2[3];
};
struct Sim3HypOut {
  int32_t count;
  float T12[16], R[9], t[3], s;
};
struct Sim3Result {
  S3Selection sel;
  float T12[16], R[9], t[3], s;
};
struct Sim3Dev {
  const Sim3Problem* prob;
  Sim3HypOut* hyp;             // all problems' hypotheses back to back
  unsigned long long* mask;    // per hypothesis `words` 64-bit words
  Sim3Result* res;
  uint8_t* inlier;             // all problems' flags back to back
};

__device__ __forceinline__ S3Point sim3_point(const Sim3Problem& pb, int i) {
  float a[3], b[3];
  if (pb.pool_form) {
    s3_transform(pb.Rcw1, pb.tcw1, pb.wpos + 3 * (size_t)pb.slot1[i], a);   // Sim3Solver.cc:107
    s3_transform(pb.Rcw2, pb.tcw2, pb.wpos + 3 * (size_t)pb.slot2[i], b);   // :110
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = pb.x1[3 * (size_t)i + c]; b[c] = pb.x2[3 * (size_t)i + c]; }
  }
  return s3_point(a, b, pb.K1, pb.K2, pb.e1[i], pb.e2[i]);
}

__global__ __launch_bounds__(256) void k_sim3_hypotheses(Sim3Dev D) {
  __shared__ float s_pt[12][kS3LdsPoints];
  const Sim3Problem& pb = D.prob[blockIdx.y];
  if ((int)blockIdx.x * kS3HypPerGroup >= pb.n_hyp) return;   // the whole workgroup, before the barrier
  const int tid = (int)threadIdx.x, n = pb.n;
  const bool lds = n <= kS3LdsPoints;
  if (lds) {
    for (int i = tid; i < n; i += 256) {
      const S3Point p = sim3_point(pb, i);
      s_pt[0][i] = p.x1[0]; s_pt[1][i] = p.x1[1]; s_pt[2][i] = p.x1[2];
      s_pt[3][i] = p.x2[0]; s_pt[4][i] = p.x2[1]; s_pt[5][i] = p.x2[2];
      s_pt[6][i] = p.p1[0]; s_pt[7][i] = p.p1[1]; s_pt[8][i] = p.p2[0]; s_pt[9][i] = p.p2[1];
      s_pt[10][i] = p.e1; s_pt[11][i] = p.e2;
    }
  }
  __syncthreads();
  const int lane = tid & 63, h = (int)blockIdx.x * kS3HypPerGroup + (tid >> 6);
  if (h >= pb.n_hyp) return;   // a whole wave; no barrier follows
  auto point = [&](int i) {
    if (!lds) return sim3_point(pb, i);
    S3Point p;
    p.x1[0] = s_pt[0][i]; p.x1[1] = s_pt[1][i]; p.x1[2] = s_pt[2][i];
    p.x2[0] = s_pt[3][i]; p.x2[1] = s_pt[4][i]; p.x2[2] = s_pt[5][i];
    p.p1[0] = s_pt[6][i]; p.p1[1] = s_pt[7][i]; p.p2[0] = s_pt[8][i]; p.p2[1] = s_pt[9][i];
    p.e1 = s_pt[10][i]; p.e2 = s_pt[11][i];
    return p;
  };
  float P1[9], P2[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const S3Point p = point(pb.samples[3 * (size_t)h + k]);   // checked by the host: inside [0, n)
#pragma unroll
    for (int c = 0; c < 3; ++c) { P1[3 * k + c] = p.x1[c]; P2[3 * k + c] = p.x2[c]; }
  }
  S3Hyp H;
  s3_compute_sim3(P1, P2, pb.fix_scale, H);
  unsigned long long* mask = D.mask + (size_t)pb.word_off + (size_t)h * (size_t)pb.words;
  int count = 0;
  for (int c = 0; c < pb.words; ++c) {   // wave-uniform
    const int i = c * 64 + lane;
    count += wave_mask_word(i < n && s3_is_inlier(H, pb.K1, pb.K2, point(i)), lane, mask + c);
  }
  if (lane == 0) {
    Sim3HypOut& o = D.hyp[(size_t)pb.hyp_off + (size_t)h];
    o.count = count;
    s3_T12(H, o.T12);
    for (int k = 0; k < 9; ++k) o.R[k] = H.R[k];
    for (int k = 0; k < 3; ++k) o.t[k] = H.t[k];
    o.s = H.s;
  }
}

__global__ __launch_bounds__(256) void k_sim3_select(Sim3Dev D) {
  __shared__ S3Selection s_sel;
  const Sim3Problem& pb = D.prob[blockIdx.x];
  if (pb.n_hyp == 0) return;   // the whole workgroup
  const int tid = (int)threadIdx.x;
  const Sim3HypOut* hyp = D.hyp + (size_t)pb.hyp_off;
  if (tid < 64) {
    // s3_select, 64 hypotheses at a time: before hypothesis k the best is max(b, c[0 .. k-1])
    int b = pb.best_inliers, held = -1, conv = 0, iters = pb.n_hyp;
    for (int base = 0; base < pb.n_hyp && !conv; base += 64) {   // wave-uniform
      const int k = base + tid;
      const bool valid = k < pb.n_hyp;
      const int c = valid ? hyp[k].count : -1;
      int m = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(m, (unsigned)d);
        if (tid >= d && o > m) m = o;
      }
      const int ex = __shfl_up(m, 1u);
      const int before = (tid == 0 || b > ex) ? b : ex;
      const bool upd = valid && c >= before;
      const bool stop = upd && c > pb.min_inliers;
      const unsigned long long su = __ballot(stop);
      unsigned long long uu = __ballot(upd);
      if (su) {
        const int first = __ffsll((long long)su) - 1;
        uu &= (2ull << first) - 1ull;
        conv = 1;
        iters = base + first + 1;
      }
      if (uu) {
        const int last = 63 - __clzll((long long)uu);
        held = base + last;
        b = __shfl(c, last);
      }
    }
    if (tid == 0) {
      S3Selection sel;
      sel.selected = held; sel.converged = conv; sel.n_inliers = held >= 0 ? b : 0; sel.iterations = iters;
      s_sel = sel;
    }
  }
  __syncthreads();
  const S3Selection sel = s_sel;
  if (tid == 0) {
    Sim3Result& r = D.res[blockIdx.x];
    r.sel = sel;
    if (sel.selected >= 0) {
      const Sim3HypOut& o = hyp[sel.selected];
      for (int k = 0; k < 16; ++k) r.T12[k] = o.T12[k];
      for (int k = 0; k < 9; ++k) r.R[k] = o.R[k];
      for (int k = 0; k < 3; ++k) r.t[k] = o.t[k];
      r.s = o.s;
    }
  }
  if (sel.selected >= 0) {
    const unsigned long long* mask = D.mask + (size_t)pb.word_off + (size_t)sel.selected * (size_t)pb.words;
    for (int i = tid; i < pb.n; i += 256) D.inlier[(size_t)pb.inl_off + i] = (uint8_t)mask_bit(mask, i);
  }
}

// ------------------------------------------------------------------------------------------------
// MLPnPsolver (src/MLPnPsolver.cpp): every RANSAC hypothesis of a call at once.  The arithmetic is csrc/mlpnp_math.h.
//   k_mlpnp_hypotheses  grid (groups of 4 hypotheses, problem), 256 work-items: one wave per hypothesis, no workgroup barrier.
//                       The wave runs the six-point computePose together (MlWaveX): the rows of A, the 12 x 12 matrix, its
//                       eigenvectors and the rows of J live in the wave's MlWork in LDS; a lane owns a correspondence, an
//                       entry of a sum, or a (row, rotation pair) of a Jacobi step; the 3 x 3 algebra and the 6 x 6 solve are
//                       wave-uniform.  Then CheckInliers over all N: a chunk's count is a ballot and a population count, the
//                       ballot word the chunk's part of the bit mask.
//   k_mlpnp_select      one workgroup per problem: ml_scan over the counts - the loop of iterate with Refine as the reference
//                       compiles it, which returns the current hypothesis (csrc/mlpnp_math.h) -, run identically by every
//                       work-item; then all work-items expand the masks of the returned hypothesis and of the record into bytes.
// Both run on the call's stream, one behind the other; no atomics, no workgroup waits for another.  Every loop is bounded.
constexpr int kMlHypPerGroup = 4;
struct MlpnpProblem {
  MlView v;
  const int32_t* samples;
  const unsigned long long* best_mask;   // the carried-in mask as bit words (null: none)
  int n_hyp;                              // 0: the problem is not run
  int min_inliers, best_inliers;
  int hyp_off, word_off, words, corr_off, cword_off;
  float best_Tcw[16];
};
struct MlpnpHypOut {
  double T[12];   // R row-major, t
  int32_t count, path;
};
struct MlpnpResult {
  MlScan scan;
  float Tcw[16], best_Tcw[16];
};
struct MlpnpDev {
  const MlpnpProblem* prob;
  MlpnpHypOut* hyp;
  unsigned long long* mask;     // per hypothesis `words` 64-bit words
  MlpnpResult* res;
  uint8_t* inlier;              // per correspondence: the flags of the returned solution
  uint8_t* best_out;            // per correspondence: the new mvbBestInliers
};

struct MlWaveX {
  int lane, lanes;
  __device__ void sync() { wave_sync(); }
  __device__ bool all(bool p) { return __ballot(!p) == 0ull; }
};
__global__ __launch_bounds__(256) void k_mlpnp_hypotheses(MlpnpDev D) {
  __shared__ MlWork s_work[kMlHypPerGroup];
  const MlpnpProblem& pb = D.prob[blockIdx.y];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = (int)blockIdx.x * kMlHypPerGroup + wave;
  if (h >= pb.n_hyp) return;   // a whole wave; the kernel has no workgroup barrier
  MlWaveX x = {lane, 64};
  MlSixSums Q;
  const MlSet S = {&pb.v, pb.samples + 6 * (size_t)h, 6};   // checked by the host: inside [0, N), distinct
  double R[9], t[3];
  int path;
  ml_compute_pose(x, s_work[wave], Q, S, R, t, &path);
  unsigned long long* mask = D.mask + (size_t)pb.word_off + (size_t)h * (size_t)pb.words;
  int count = 0;
  for (int c = 0; c < pb.words; ++c) {   // wave-uniform
    const int i = c * 64 + lane;
    count += wave_mask_word(i < pb.v.N && ml_is_inlier(pb.v, R, t, i), lane, mask + c);
  }
  if (lane == 0) {
    MlpnpHypOut& o = D.hyp[(size_t)pb.hyp_off + (size_t)h];
    for (int k = 0; k < 9; ++k) o.T[k] = R[k];
    for (int k = 0; k < 3; ++k) o.T[9 + k] = t[k];
    o.count = count;
    o.path = path;
  }
}

__global__ __launch_bounds__(256) void k_mlpnp_select(MlpnpDev D) {
  const MlpnpProblem& pb = D.prob[blockIdx.x];
  if (pb.n_hyp == 0) return;   // the whole workgroup
  const int tid = (int)threadIdx.x, N = pb.v.N, words = pb.words;
  const MlpnpHypOut* hyp = D.hyp + (size_t)pb.hyp_off;
  const unsigned long long* masks = D.mask + (size_t)pb.word_off;
  struct Counts {   // c[k] of ml_scan
    const MlpnpHypOut* h;
    __device__ int operator[](int k) const { return h[k].count; }
  };
  const MlScan sc = ml_scan(Counts{hyp}, pb.n_hyp, pb.min_inliers, pb.best_inliers);   // wave-uniform loads, the same in every work-item
  // mvbBestInliers: the record's mask, or the one carried in; what iterate hands out: the stopping hypothesis's, or the best
  const unsigned long long* bm = sc.record >= 0 ? masks + (size_t)sc.record * (size_t)words : (pb.best_inliers > 0 ? pb.best_mask : nullptr);
  const unsigned long long* om = sc.selected >= 0 ? masks + (size_t)sc.selected * (size_t)words : bm;
  for (int i = tid; i < N; i += 256) {
    if (bm) D.best_out[(size_t)pb.corr_off + i] = (uint8_t)mask_bit(bm, i);
    if (sc.found) D.inlier[(size_t)pb.corr_off + i] = (uint8_t)mask_bit(om, i);
  }
  if (tid == 0) {
    MlpnpResult& r = D.res[blockIdx.x];
    r.scan = sc;
    if (sc.record >= 0) ml_Tcw(hyp[sc.record].T, hyp[sc.record].T + 9, r.best_Tcw);
    else for (int k = 0; k < 16; ++k) r.best_Tcw[k] = pb.best_Tcw[k];
    if (sc.selected >= 0) ml_Tcw(hyp[sc.selected].T, hyp[sc.selected].T + 9, r.Tcw);
    else for (int k = 0; k < 16; ++k) r.Tcw[k] = r.best_Tcw[k];
  }
}

// ------------------------------------------------------------------------------------------------
// TwoViewReconstruction (src/TwoViewReconstruction.cc): every homography and every fundamental hypothesis of a call at once.
// The arithmetic is csrc/twoview_math.h.
//   k_tv_normalize    grid (2 frames, problem), one wave: Normalize over ALL keys of the frame.  The wave stages 64 keys in LDS,
//                     then every lane adds the two serial chains in index order.
//   k_tv_hypotheses   grid (groups of 4 hypotheses, 2 models, problem), 256 work-items: one wave per (hypothesis, model), no
//                     workgroup barrier.  The wave fills A from its eight matches, runs the Jacobi in its TvWork in LDS and forms
//                     H21i / H12i or F21i wave-uniformly; then walks the matches 64 at a time: a lane computes both terms of
//                     its match and its inlier bit, the chunk's mask word is a ballot, and the 128 terms go through LDS to be
//                     added by every lane in the reference's order (two per match, ascending match index): no tree.
//   k_tv_select       one workgroup per problem: the first strictly greater score per model, Reconstruct's choice, the inlier
//                     count of the chosen mask, the motion hypotheses (DecomposeE, or Faugeras' eight with the d1 / d2, d2 / d3
//                     exit); all work-items expand the two winners' masks into bytes.
//   k_tv_check_rt     grid (8 motion hypotheses, problem), 256 work-items: CheckRT over the inliers of the chosen model.  nGood is
//                     an integer tree; the min(50, nGood - 1)-th smallest cosParallax comes from at most 51 rounds of "smallest
//                     value above the last one, and how often" (an order-free min / count tree each).
//   k_tv_decide       one workgroup per problem: the rules of ReconstructF / ReconstructH, T21, and the winning hypothesis's
//                     points and flags copied out.
// All run on the call's stream, one behind the other; no floating-point atomics, no workgroup waits for another, every loop
// is bounded.
constexpr int kTvHypPerGroup = 4;
struct TvProblem {
  TvView v;                 // T1 / T2 come from k_tv_normalize
  const int32_t* samples;
  int n_hyp;                // 0: the problem is not run
  int words, hyp_off, match_off, key_off;
  unsigned long long word_off;
};
struct TvSelect {
  float SH, SF;
  int32_t best_h, best_f, model, n_inliers, exit_code;
  float H21[9], F21[9];
  TvMotions mo;
};
struct TvResult {
  int32_t found, model, exit_code, best, aux, n_inliers, best_h, best_f;
  float SH, SF, H21[9], F21[9], R[9], t[3];
  int32_t n_good[kTvMaxMotions];
  float parallax[kTvMaxMotions];
};
struct TvDev {
  const TvProblem* prob;
  float* norm;                  // per problem 2 x (sX, sY, meanX, meanY)
  float* score;                 // per hypothesis 2
  float* model;                 // per hypothesis 2 x 9
  unsigned long long* mask;     // per hypothesis 2 x `words` 64-bit words
  TvSelect* sel;
  int32_t* n_good;              // per problem 8
  float* parallax;              // per problem 8
  float* cosv;                  // per problem 8 x N: the vCosParallax entry of a counted match, else NaN
  float* p3d;                   // per problem 8 x n1 x 3
  uint8_t* good;                // per problem 8 x n1
  TvResult* res;
  float* p3d_out;               // per problem n1 x 3
  uint8_t* tri_out;             // per problem n1
  uint8_t *mask_h, *mask_f;     // per match: the winners' inlier flags
};
__device__ __forceinline__ TvView tv_view(const TvDev& D, const TvProblem& pb, int b) {
  TvView v = pb.v;
  for (int k = 0; k < 4; ++k) { v.T1[k] = D.norm[8 * (size_t)b + k]; v.T2[k] = D.norm[8 * (size_t)b + 4 + k]; }
  return v;
}

__global__ __launch_bounds__(64) void k_tv_normalize(TvDev D) {
  __shared__ float s_buf[2][64];
  const TvProblem& pb = D.prob[blockIdx.y];
  if (pb.n_hyp == 0) return;   // the whole wave
  MlWaveX x = {(int)threadIdx.x, 64};
  const int f = (int)blockIdx.x;
  float T[4];
  tv_normalize(x, s_buf, f ? pb.v.xy2 : pb.v.xy1, f ? pb.v.n2 : pb.v.n1, T);
  if (threadIdx.x == 0) {   // every lane holds the same T; constant indices keep it in registers (T[threadIdx.x] would put it into scratch)
    float* out = D.norm + 8 * (size_t)blockIdx.y + 4 * f;
    out[0] = T[0]; out[1] = T[1]; out[2] = T[2]; out[3] = T[3];
  }
}

__global__ __launch_bounds__(256) void k_tv_hypotheses(TvDev D) {
  __shared__ TvWork s_work[kTvHypPerGroup];
  const TvProblem& pb = D.prob[blockIdx.z];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = (int)blockIdx.x * kTvHypPerGroup + wave, model = (int)blockIdx.y;
  if (h >= pb.n_hyp) return;   // a whole wave; the kernel has no workgroup barrier
  const TvView v = tv_view(D, pb, (int)blockIdx.z);
  TvWork& W = s_work[wave];
  MlWaveX x = {lane, 64};
  float M[9], M2[9];
  tv_model(x, W, v, pb.samples + 8 * (size_t)h, model, M, M2);   // the sets are checked by the host: inside [0, N), distinct
  const float invSigmaSquare = tv_inv_sigma2(v.sigma);
  const size_t hm = 2 * ((size_t)pb.hyp_off + (size_t)h) + (size_t)model;
  unsigned long long* mask = D.mask + pb.word_off + (2 * (size_t)h + (size_t)model) * (size_t)pb.words;
  float score = 0.0f;
  for (int c = 0; c < pb.words; ++c) {   // wave-uniform
    const int i = c * 64 + lane;
    float t[2] = {0.0f, 0.0f};
    bool in = false;
    if (i < v.N) in = tv_check(model, M, M2, v, i, invSigmaSquare, t);
    W.terms[2 * lane] = t[0];
    W.terms[2 * lane + 1] = t[1];
    wave_sync();
    score = tv_add_chunk(score, W.terms, 128);   // past N the terms are +0.0f
    wave_sync();
    (void)wave_mask_word(in, lane, mask + c);
  }
  if (lane == 0) {
    D.score[hm] = score;
    for (int k = 0; k < 9; ++k) D.model[9 * hm + k] = M[k];
  }
}

__global__ __launch_bounds__(256) void k_tv_select(TvDev D) {
  __shared__ int s_cnt[256];
  const TvProblem& pb = D.prob[blockIdx.x];
  if (pb.n_hyp == 0) return;   // the whole workgroup
  const int tid = (int)threadIdx.x, N = pb.v.N, words = pb.words;
  const float* scores = D.score + 2 * (size_t)pb.hyp_off;
  float SH, SF;   // wave-uniform loads, the same in every work-item
  const int best_h = tv_first_max(scores, pb.n_hyp, 0, &SH), best_f = tv_first_max(scores, pb.n_hyp, 1, &SF);
  const int model = tv_choose_model(SH, SF);
  const unsigned long long* mh = best_h >= 0 ? D.mask + pb.word_off + (2 * (size_t)best_h) * (size_t)words : nullptr;
  const unsigned long long* mf = best_f >= 0 ? D.mask + pb.word_off + (2 * (size_t)best_f + 1) * (size_t)words : nullptr;
  const unsigned long long* chosen = model == 0 ? mh : mf;   // model >= 0 has a score > 0 on that side: a winner
  int cnt = 0;
  for (int c = tid; model >= 0 && c < words; c += 256) cnt += __popcll(chosen[c]);
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) s_cnt[tid] += s_cnt[tid + s];
    __syncthreads();
  }
  for (int i = tid; i < N; i += 256) {
    D.mask_h[(size_t)pb.match_off + i] = mh ? (uint8_t)mask_bit(mh, i) : (uint8_t)0;
    D.mask_f[(size_t)pb.match_off + i] = mf ? (uint8_t)mask_bit(mf, i) : (uint8_t)0;
  }
  if (tid == 0) {
    TvSelect& S = D.sel[blockIdx.x];
    S.SH = SH; S.SF = SF; S.best_h = best_h; S.best_f = best_f; S.model = model; S.n_inliers = s_cnt[0];
    for (int k = 0; k < 9; ++k) {
      S.H21[k] = best_h >= 0 ? D.model[9 * (2 * ((size_t)pb.hyp_off + (size_t)best_h)) + k] : 0.0f;
      S.F21[k] = best_f >= 0 ? D.model[9 * (2 * ((size_t)pb.hyp_off + (size_t)best_f) + 1) + k] : 0.0f;
    }
    S.exit_code = kTvFound;
    if (model < 0) {
      S.exit_code = kTvNoScore;
      S.mo.n = 0;
    } else if (model == 0) {
      if (!tv_motions_h(S.H21, pb.v.K, S.mo)) S.exit_code = kTvHRatio;
    } else {
      tv_motions_f(S.F21, pb.v.K, S.mo);
    }
  }
}

__global__ __launch_bounds__(256) void k_tv_check_rt(TvDev D) {
  __shared__ int s_cnt[256];
  __shared__ float s_val[256];
  const int b = (int)blockIdx.y, j = (int)blockIdx.x, tid = (int)threadIdx.x;
  const TvProblem& pb = D.prob[b];
  if (pb.n_hyp == 0) return;   // the whole workgroup
  const TvSelect& S = D.sel[b];
  const int N = pb.v.N, n1 = pb.v.n1;
  if (j >= S.mo.n) {           // the whole workgroup
    if (tid == 0) { D.n_good[8 * (size_t)b + j] = 0; D.parallax[8 * (size_t)b + j] = 0.0f; }
    return;
  }
  TvCam c;
  tv_cam(pb.v.K, S.mo.R[j], S.mo.t[j], pb.v.sigma, c);
  float* p3d = D.p3d + 3 * (8 * (size_t)pb.key_off + (size_t)j * (size_t)n1);
  uint8_t* good = D.good + 8 * (size_t)pb.key_off + (size_t)j * (size_t)n1;
  float* cosv = D.cosv + 8 * (size_t)pb.match_off + (size_t)j * (size_t)N;
  for (int i = tid; i < n1; i += 256) { p3d[3 * (size_t)i] = 0.0f; p3d[3 * (size_t)i + 1] = 0.0f; p3d[3 * (size_t)i + 2] = 0.0f; good[i] = 0; }
  __syncthreads();
  const unsigned long long* mask = D.mask + pb.word_off + (2 * (size_t)(S.model == 0 ? S.best_h : S.best_f) + (size_t)S.model) * (size_t)pb.words;
  const float nan = np_float(0x7fc00000u);
  int cnt = 0;
  for (int i = tid; i < N; i += 256) {
    float cv = nan;
    if (mask_bit(mask, i)) {
      const size_t a = (size_t)pb.v.m1[i], q = (size_t)pb.v.m2[i];   // the matches name distinct keys of frame 1
      float p[3], cp;
      const int code = tv_rt_point(c, pb.v.xy1[2 * a], pb.v.xy1[2 * a + 1], pb.v.xy2[2 * q], pb.v.xy2[2 * q + 1], p, &cp);
      if (code) {
        p3d[3 * a] = p[0]; p3d[3 * a + 1] = p[1]; p3d[3 * a + 2] = p[2];
        good[a] = code == 2 ? 1 : 0;
        cv = cp;
        ++cnt;
      }
    }
    cosv[i] = cv;   // read back by this work-item only
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) s_cnt[tid] += s_cnt[tid + s];
    __syncthreads();
  }
  const int nGood = s_cnt[0];
  __syncthreads();
  // sort + vCosParallax[min(50, size - 1)]: the values in ascending order, one distinct value per round
  const int idx = nGood - 1 < 50 ? nGood - 1 : 50;
  float last = 0.0f, pick = nan;
  int rank = 0;
  for (int round = 0; nGood > 0 && round <= idx; ++round) {   // uniform: at most 51 rounds
    float lo = nan;
    int m = 0;
    for (int i = tid; i < N; i += 256) {
      const float cv = cosv[i];
      if (!(cv == cv) || (round > 0 && !(cv > last))) continue;
      if (m == 0 || cv < lo) { lo = cv; m = 1; }
      else if (cv == lo) ++m;
    }
    s_val[tid] = lo;
    s_cnt[tid] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (tid < s) {
        const float a = s_val[tid], o = s_val[tid + s];
        const int ma = s_cnt[tid], mo = s_cnt[tid + s];
        if (mo > 0 && (ma == 0 || o < a)) { s_val[tid] = o; s_cnt[tid] = mo; }
        else if (mo > 0 && o == a) s_cnt[tid] = ma + mo;
      }
      __syncthreads();
    }
    const float v0 = s_val[0];
    const int m0 = s_cnt[0];
    __syncthreads();
    if (m0 == 0) break;                              // only NaN values are left: pick stays NaN
    if (rank + m0 > idx) { pick = v0; break; }
    rank += m0;
    last = v0;
  }
  if (tid == 0) {
    D.n_good[8 * (size_t)b + j] = nGood;
    D.parallax[8 * (size_t)b + j] = nGood > 0 ? tv_parallax_deg(pick) : 0.0f;
  }
}

__global__ __launch_bounds__(256) void k_tv_decide(TvDev D) {
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
  const TvProblem& pb = D.prob[b];
  if (pb.n_hyp == 0) return;   // the whole workgroup
  const TvSelect& S = D.sel[b];
  int32_t nGood[kTvMaxMotions];
  float parallax[kTvMaxMotions];
  for (int k = 0; k < kTvMaxMotions; ++k) { nGood[k] = D.n_good[8 * (size_t)b + k]; parallax[k] = D.parallax[8 * (size_t)b + k]; }
  TvDecision d = {0, S.exit_code, -1, 0};   // the same in every work-item
  if (S.exit_code == kTvFound) d = S.model == 0 ? tv_decide_h(nGood, parallax, S.n_inliers) : tv_decide_f(nGood, parallax, S.n_inliers);
  const int n1 = pb.v.n1;
  if (d.found) {
    const float* p3d = D.p3d + 3 * (8 * (size_t)pb.key_off + (size_t)d.best * (size_t)n1);
    const uint8_t* good = D.good + 8 * (size_t)pb.key_off + (size_t)d.best * (size_t)n1;
    for (int i = tid; i < n1; i += 256) {
      for (int k = 0; k < 3; ++k) D.p3d_out[3 * ((size_t)pb.key_off + i) + k] = p3d[3 * (size_t)i + k];
      D.tri_out[(size_t)pb.key_off + i] = good[i];
    }
  }
  if (tid == 0) {
    TvResult& r = D.res[b];
    r.found = d.found; r.model = S.model; r.exit_code = d.exit_code; r.best = d.best; r.aux = d.aux; r.n_inliers = S.n_inliers;
    r.best_h = S.best_h; r.best_f = S.best_f; r.SH = S.SH; r.SF = S.SF;
    for (int k = 0; k < 9; ++k) { r.H21[k] = S.H21[k]; r.F21[k] = S.F21[k]; r.R[k] = d.found ? S.mo.R[d.best][k] : ((k % 4 == 0) ? 1.0f : 0.0f); }
    for (int k = 0; k < 3; ++k) r.t[k] = d.found ? S.mo.t[d.best][k] : 0.0f;
    for (int k = 0; k < kTvMaxMotions; ++k) { r.n_good[k] = nGood[k]; r.parallax[k] = parallax[k]; }
  }
}

}  // namespace rgbl

using namespace rgbl;

extern "C" {

// ---- Sim3Solver (src/Sim3Solver.cc) ------------------------------------------------------------------------------------
namespace {
// a sample: k distinct indices in [0, N)
bool distinct_in_range(const int32_t* s, int k, int N) {
  for (int i = 0; i < k; ++i) {
    if (s[i] < 0 || s[i] >= N) return false;
    for (int j = 0; j < i; ++j)
      if (s[i] == s[j]) return false;
  }
  return true;
}
// Where the problems of a batch that run put their hypotheses, their mask words (`masks` bit masks of ceil(items / 64) words per
// hypothesis) and their items (at most 65535 each: B < 2^15 problems fit an int), back to back.  add() refuses a problem that
// takes the hypotheses past hyp_cap; the cap on the words and both messages are the caller's.
struct BatchOffsets {
  std::vector<int> hyp, item;
  std::vector<size_t> word;
  int max_hyp = 0;
  explicit BatchOffsets(int B) : hyp((size_t)B + 1, 0), item((size_t)B + 1, 0), word((size_t)B + 1, 0) {}
  bool add(int b, int nh, int nn, int masks, int hyp_cap) {
    if (hyp[(size_t)b] > hyp_cap - nh) return false;
    hyp[(size_t)b + 1] = hyp[(size_t)b] + nh;
    item[(size_t)b + 1] = item[(size_t)b] + nn;
    word[(size_t)b + 1] = word[(size_t)b] + (size_t)masks * (size_t)nh * (size_t)((nn + 63) / 64);
    max_hyp = std::max(max_hyp, nh);
    return true;
  }
};
constexpr int kS3MaxHyp = 1 << 20;
// a problem the reference leaves at once (:155-159), or that has nothing to run
inline bool sim3_skipped(const rgbl_sim3_input* in) { return in->n < 3 || in->n < in->min_inliers || in->n_hyp == 0; }
// everything that can be refused without the pool is refused here, before anything is staged, launched or written
int check_sim3_input(const rgbl_sim3_input* in, int b, bool host_only) {
  if (in->n < 0 || in->n > 65535 || in->n_hyp < 0 || in->n_hyp > kS3MaxHyp) { set_error("sim3 %d: n outside [0, 65535] or n_hyp outside [0, %d]", b, kS3MaxHyp); return RGBL_ERR_INVALID; }
  if (host_only && in->pool) { set_error("sim3 %d: the host build reads host arrays only", b); return RGBL_ERR_INVALID; }
  if (in->n > 0 && (in->pool ? (!in->slot1 || !in->slot2) : (!in->x1c || !in->x2c))) { set_error("sim3 %d: the points are either x1c, x2c or a pool with slot1, slot2", b); return RGBL_ERR_INVALID; }
  if (in->n > 0 && (!in->max_err1 || !in->max_err2)) { set_error("sim3 %d: no max_err1 / max_err2", b); return RGBL_ERR_INVALID; }
  bool finite = true;
  for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->K1[i]) && std::isfinite(in->K2[i]);
  if (in->pool) {
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(in->Rcw1[i]) && std::isfinite(in->Rcw2[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(in->tcw1[i]) && std::isfinite(in->tcw2[i]);
  }
  for (int i = 0; i < in->n; ++i) finite = finite && std::isfinite(in->max_err1[i]) && std::isfinite(in->max_err2[i]);
  if (!finite) { set_error("sim3 %d: K, a pose or a threshold is not finite", b); return RGBL_ERR_INVALID; }
  if (in->n >= 3 && in->n_hyp > 0) {
    if (!in->samples) { set_error("sim3 %d: no samples", b); return RGBL_ERR_INVALID; }
    for (int k = 0; k < in->n_hyp; ++k) {
      const int32_t* s = in->samples + 3 * (size_t)k;
      if (!distinct_in_range(s, 3, in->n)) {
        set_error("sim3 %d: sample %d = (%d, %d, %d) is not three distinct indices in [0, %d)", b, k, s[0], s[1], s[2], in->n);
        return RGBL_ERR_INVALID;
      }
    }
  }
  return RGBL_OK;
}
void write_sim3_output(const rgbl_sim3_input* in, rgbl_sim3_output* out, const Sim3Result& r, const uint8_t* inlier, const Sim3HypOut* hyp) {
  out->selected = r.sel.selected; out->converged = r.sel.converged; out->n_inliers = r.sel.n_inliers; out->iterations_run = r.sel.iterations;
  if (r.sel.selected >= 0) {
    memcpy(out->T12, r.T12, sizeof(out->T12)); memcpy(out->R12, r.R, sizeof(out->R12)); memcpy(out->t12, r.t, sizeof(out->t12));
    out->s12 = r.s;
    if (out->inlier && in->n) memcpy(out->inlier, inlier, (size_t)in->n);
  }
  for (int k = 0; k < in->n_hyp; ++k) {
    if (out->counts) out->counts[k] = hyp[k].count;
    if (out->T12_all) memcpy(out->T12_all + 16 * (size_t)k, hyp[k].T12, sizeof(hyp[k].T12));
  }
}
}  // namespace

int rgbl_sim3_ransac_host(const rgbl_sim3_input* in, rgbl_sim3_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  RGBL_TRY(check_sim3_input(in, 0, true));
  if (sim3_skipped(in)) { out->selected = -1; return RGBL_OK; }
  const int n = in->n, words = (n + 63) / 64;
  std::vector<S3Point> pts((size_t)n);
  for (int i = 0; i < n; ++i) pts[(size_t)i] = s3_point(in->x1c + 3 * (size_t)i, in->x2c + 3 * (size_t)i, in->K1, in->K2, in->max_err1[i], in->max_err2[i]);
  std::vector<Sim3HypOut> hyp((size_t)in->n_hyp);
  std::vector<int32_t> counts((size_t)in->n_hyp);
  std::vector<unsigned long long> mask((size_t)in->n_hyp * (size_t)words, 0ull);
  for (int h = 0; h < in->n_hyp; ++h) {
    float P1[9], P2[9];
    for (int k = 0; k < 3; ++k) {
      const S3Point& p = pts[(size_t)in->samples[3 * (size_t)h + k]];
      for (int c = 0; c < 3; ++c) { P1[3 * k + c] = p.x1[c]; P2[3 * k + c] = p.x2[c]; }
    }
    S3Hyp H;
    s3_compute_sim3(P1, P2, in->fix_scale, H);
    int count = 0;
    for (int i = 0; i < n; ++i)
      if (s3_is_inlier(H, in->K1, in->K2, pts[(size_t)i])) { mask[(size_t)h * words + (i >> 6)] |= 1ull << (i & 63); ++count; }
    Sim3HypOut& o = hyp[(size_t)h];
    o.count = counts[(size_t)h] = count;
    s3_T12(H, o.T12);
    memcpy(o.R, H.R, sizeof(o.R)); memcpy(o.t, H.t, sizeof(o.t));
    o.s = H.s;
  }
  Sim3Result r;
  memset(&r, 0, sizeof(r));
  r.sel = s3_select(counts.data(), in->n_hyp, in->best_inliers, in->min_inliers);
  std::vector<uint8_t> inl((size_t)n, 0);
  if (r.sel.selected >= 0) {
    const Sim3HypOut& o = hyp[(size_t)r.sel.selected];
    memcpy(r.T12, o.T12, sizeof(r.T12)); memcpy(r.R, o.R, sizeof(r.R)); memcpy(r.t, o.t, sizeof(r.t));
    r.s = o.s;
    for (int i = 0; i < n; ++i) inl[(size_t)i] = (uint8_t)mask_bit(mask.data() + (size_t)r.sel.selected * words, i);
  }
  write_sim3_output(in, out, r, inl.data(), hyp.data());
  return RGBL_OK;
}

int rgbl_sim3_ransac_batch(rgbl_matcher* m, int n_problems, const rgbl_sim3_input* in, rgbl_sim3_output* out) {
  if (!m || n_problems < 0 || (n_problems > 0 && (!in || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int B = n_problems;
  if (B > 32767) { set_error("sim3: more than 32767 problems in one call"); return RGBL_ERR_INVALID; }
  PoolCall pc(m, "sim3", "a frame");
  BatchOffsets off(B);   // of the problems that run: hypotheses, mask words, flags
  for (int b = 0; b < B; ++b) {
    RGBL_TRY(check_sim3_input(in + b, b, false));
    RGBL_TRY(pc.note(in[b].pool, {}, b));
    const bool run = !sim3_skipped(in + b);
    const int nh = run ? in[b].n_hyp : 0, nn = run ? in[b].n : 0;
    if (!off.add(b, nh, nn, 1, INT_MAX)) { set_error("sim3: more than 2^31 hypotheses in one call"); return RGBL_ERR_INVALID; }
  }
  if (off.word[(size_t)B] > (size_t)INT_MAX) { set_error("sim3: more than 2^31 mask words in one call"); return RGBL_ERR_INVALID; }
  const rgbl_map_points* pool = pc.pool;
  RGBL_TRY(pc.lock(B, [&](int b) -> int {
    for (int i = 0; in[b].pool && i < in[b].n; ++i)
      if (!pc.holds(in[b].slot1[i]) || !pc.holds(in[b].slot2[i])) {
        set_error("sim3 %d: slots (%d, %d) of correspondence %d outside [0, %d)", b, in[b].slot1[i], in[b].slot2[i], i, pool->cap);
        return RGBL_ERR_INVALID;
      }
    return RGBL_OK;
  }));
  const int H = off.hyp[(size_t)B];
  if (H == 0) {   // nothing to run (B == 0 included)
    for (int b = 0; b < B; ++b) out[b].selected = -1;
    return RGBL_OK;
  }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // behind pc (PoolCall)
  HostCall hc(m);
  hipStream_t s = hc.s;
  std::vector<Sim3Problem> prob((size_t)B);
  Sim3Dev D;
  memset(&D, 0, sizeof(D));
  bool diag = false;
  for (int b = 0; b < B; ++b) diag = diag || out[b].counts || out[b].T12_all;
  RGBL_TRY(hc.begin([&]() -> int {
    for (int b = 0; b < B; ++b) {
      Sim3Problem& P = prob[(size_t)b];
      memset(&P, 0, sizeof(P));
      const rgbl_sim3_input& I = in[b];
      if (sim3_skipped(&I)) continue;   // n_hyp = 0: no workgroup touches it
      if (I.pool) {
        P.pool_form = 1; P.wpos = pool->d_wpos;
        hc.put(&P.slot1, I.slot1, (size_t)I.n);
        hc.put(&P.slot2, I.slot2, (size_t)I.n);
        memcpy(P.Rcw1, I.Rcw1, sizeof(P.Rcw1)); memcpy(P.tcw1, I.tcw1, sizeof(P.tcw1));
        memcpy(P.Rcw2, I.Rcw2, sizeof(P.Rcw2)); memcpy(P.tcw2, I.tcw2, sizeof(P.tcw2));
      } else {
        hc.put(&P.x1, I.x1c, (size_t)I.n * 3);
        hc.put(&P.x2, I.x2c, (size_t)I.n * 3);
      }
      hc.put(&P.e1, I.max_err1, (size_t)I.n);
      hc.put(&P.e2, I.max_err2, (size_t)I.n);
      hc.put(&P.samples, I.samples, (size_t)I.n_hyp * 3);
      P.n = I.n; P.n_hyp = I.n_hyp; P.words = (I.n + 63) / 64;
      P.hyp_off = off.hyp[(size_t)b]; P.word_off = (int)off.word[(size_t)b]; P.inl_off = off.item[(size_t)b];
      P.fix_scale = I.fix_scale ? 1 : 0; P.min_inliers = I.min_inliers; P.best_inliers = I.best_inliers;
      memcpy(P.K1, I.K1, sizeof(P.K1)); memcpy(P.K2, I.K2, sizeof(P.K2));
    }
    D.prob = hc.stage<Sim3Problem>((size_t)B, [&](Sim3Problem* dst) { memcpy(dst, prob.data(), sizeof(Sim3Problem) * (size_t)B); });
    D.res = hc.result<Sim3Result>((size_t)B);   // what comes back, side by side
    D.inlier = hc.result<uint8_t>((size_t)off.item[(size_t)B]);
    D.hyp = diag ? hc.result<Sim3HypOut>((size_t)H) : hc.scratch<Sim3HypOut>((size_t)H);
    D.mask = hc.scratch<unsigned long long>(off.word[(size_t)B]);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_sim3_hypotheses", k_sim3_hypotheses, dim3((unsigned)((off.max_hyp + kS3HypPerGroup - 1) / kS3HypPerGroup), (unsigned)B), dim3(256), 0, D));
  RGBL_TRY(launch(m, s, "k_sim3_select", k_sim3_select, dim3((unsigned)B), dim3(256), 0, D));
  RGBL_TRY(hc.fetch());
  for (int b = 0; b < B; ++b) {
    if (sim3_skipped(in + b)) { out[b].selected = -1; continue; }
    write_sim3_output(in + b, out + b, hc.host(D.res)[b], hc.host(D.inlier) + off.item[(size_t)b], hc.host(D.hyp) + off.hyp[(size_t)b]);
  }
  return RGBL_OK;
}

int rgbl_sim3_ransac(rgbl_matcher* m, const rgbl_sim3_input* in, rgbl_sim3_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return rgbl_sim3_ransac_batch(m, 1, in, out);
}

// ---- MLPnPsolver (src/MLPnPsolver.cpp) ------------------------------------------------------------------------------------
namespace {
constexpr int kMlMaxHyp = 1 << 20;
constexpr int kMlMaxMaskWordsLog2 = 26;   // 512 MB of masks: 2^20 hypotheses of 4096 correspondences, or 65535 correspondences of 65536 hypotheses
constexpr size_t kMlMaxMaskWords = (size_t)1 << kMlMaxMaskWordsLog2;
// Everything that can be refused without the pool is refused here, before anything is staged, launched or written.  *n_corr = N.
int check_mlpnp_input(const rgbl_mlpnp_input* in, int b, bool host_only, int* n_corr) {
  *n_corr = 0;
  if (in->n < 0 || in->n > 65535 || in->n_hyp < 0 || in->n_hyp > kMlMaxHyp) { set_error("mlpnp %d: n outside [0, 65535] or n_hyp outside [0, %d]", b, kMlMaxHyp); return RGBL_ERR_INVALID; }
  if (in->n_points < 0 || (in->n > 0 && !in->mp_index)) { set_error("mlpnp %d: n_points < 0 or no mp_index", b); return RGBL_ERR_INVALID; }
  if (in->min_inliers < 6) { set_error("mlpnp %d: min_inliers %d < 6, the minimal set", b, in->min_inliers); return RGBL_ERR_INVALID; }
  if (in->n_levels < 1 || in->n_levels > kProjMaxLevels || !in->level_sigma2) { set_error("mlpnp %d: n_levels outside [1, %d] or no level_sigma2", b, kProjMaxLevels); return RGBL_ERR_INVALID; }
  bool finite = std::isfinite(in->th2);
  for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->K[i]);
  for (int i = 0; i < in->n_levels; ++i) finite = finite && std::isfinite(in->level_sigma2[i]);
  if (!finite) { set_error("mlpnp %d: K, th2 or a sigma2 is not finite", b); return RGBL_ERR_INVALID; }
  if (host_only && (in->device || in->pool)) { set_error("mlpnp %d: the host build reads host arrays only", b); return RGBL_ERR_INVALID; }
  if (in->device ? in->device->n != in->n : (in->n > 0 && (!in->kp_xy || !in->kp_octave))) {
    set_error("mlpnp %d: the frame side is either kp_xy, kp_octave or a resident frame of n features", b);
    return RGBL_ERR_INVALID;
  }
  if (in->n_points > 0 && (in->pool ? !in->slot : !in->world_pos)) { set_error("mlpnp %d: the map side is either world_pos or a pool with slot", b); return RGBL_ERR_INVALID; }
  int N = 0;
  RGBL_TRY(check_correspondences("mlpnp", b, in->n, in->mp_index, in->n_points, in->device ? nullptr : in->kp_octave, in->n_levels, &N));
  if (in->best_inliers < 0) { set_error("mlpnp %d: best_inliers < 0", b); return RGBL_ERR_INVALID; }
  if (in->best_inliers > 0) {
    int ones = 0;
    for (int i = 0; in->best_mask && i < N; ++i) ones += in->best_mask[i] ? 1 : 0;
    if (!in->best_mask || ones != in->best_inliers || ones < 6) { set_error("mlpnp %d: best_inliers = %d needs a best_mask with as many (>= 6) ones", b, in->best_inliers); return RGBL_ERR_INVALID; }
  }
  if (N >= in->min_inliers && in->n_hyp > 0) {
    if (N < 6) { set_error("mlpnp %d: %d correspondences, a sample needs 6", b, N); return RGBL_ERR_INVALID; }
    if (!in->samples) { set_error("mlpnp %d: no samples", b); return RGBL_ERR_INVALID; }
    for (int k = 0; k < in->n_hyp; ++k) {
      const int32_t* s = in->samples + 6 * (size_t)k;
      if (!distinct_in_range(s, 6, N)) { set_error("mlpnp %d: sample %d = (%d, %d, %d, %d, %d, %d) is not six distinct indices in [0, %d)", b, k, s[0], s[1], s[2], s[3], s[4], s[5], N); return RGBL_ERR_INVALID; }
    }
  }
  *n_corr = N;
  return RGBL_OK;
}
// a problem the reference leaves at once (:106-110), or that has nothing to run
inline bool mlpnp_skipped(const rgbl_mlpnp_input* in, int N) { return N < in->min_inliers || in->n_hyp == 0; }
void write_mlpnp_skipped(const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out, int N) {
  out->found = 0; out->no_more = N < in->min_inliers ? 1 : 0; out->n_inliers = 0; out->iterations_run = 0; out->refines = 0;
  for (int k = 0; k < 16; ++k) out->Tcw[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  out->best_inliers = in->best_inliers;
  memcpy(out->best_Tcw, in->best_Tcw, sizeof(out->best_Tcw));
  if (out->best_mask && in->best_inliers > 0) memcpy(out->best_mask, in->best_mask, (size_t)N);
}
// inlier / best: per correspondence
void write_mlpnp_output(const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out, int N, const MlpnpResult& r, const uint8_t* inlier, const uint8_t* best,
                        const MlpnpHypOut* hyp) {
  const MlScan& sc = r.scan;
  out->found = sc.found; out->no_more = sc.no_more; out->n_inliers = sc.n_inliers; out->iterations_run = sc.iterations; out->refines = sc.refines;
  if (sc.found) memcpy(out->Tcw, r.Tcw, sizeof(out->Tcw));
  else for (int k = 0; k < 16; ++k) out->Tcw[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  if (sc.found && out->inlier) {
    memset(out->inlier, 0, (size_t)in->n);
    int k = 0;
    for (int i = 0; i < in->n; ++i)
      if (in->mp_index[i] >= 0) out->inlier[i] = inlier[k++];
  }
  out->best_inliers = sc.best;
  memcpy(out->best_Tcw, r.best_Tcw, sizeof(out->best_Tcw));
  if (out->best_mask && sc.best > 0) memcpy(out->best_mask, best, (size_t)N);
  for (int k = 0; hyp && k < in->n_hyp; ++k) {
    if (out->counts) out->counts[k] = hyp[k].count;
    if (out->gn_path) out->gn_path[k] = hyp[k].path;
    if (out->Tcw_all) {
      double* T = out->Tcw_all + 12 * (size_t)k;
      for (int i = 0; i < 3; ++i) { T[4 * i] = hyp[k].T[3 * i]; T[4 * i + 1] = hyp[k].T[3 * i + 1]; T[4 * i + 2] = hyp[k].T[3 * i + 2]; T[4 * i + 3] = hyp[k].T[9 + i]; }
    }
  }
}
// the correspondences of a problem: feature and row of the map side
void mlpnp_correspondences(const rgbl_mlpnp_input* in, int32_t* feat, int32_t* point) {
  list_correspondences(in->n, in->mp_index, in->pool ? in->slot : nullptr, feat, point);
}
void mlpnp_mask_words(const uint8_t* bytes, int N, unsigned long long* words) {
  for (int w = 0; w < (N + 63) / 64; ++w) words[w] = 0;
  for (int i = 0; i < N; ++i)
    if (bytes[i]) words[i >> 6] |= 1ull << (i & 63);
}
}  // namespace

int rgbl_mlpnp_ransac_host(const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  int N = 0;
  RGBL_TRY(check_mlpnp_input(in, 0, true, &N));
  if (mlpnp_skipped(in, N)) { write_mlpnp_skipped(in, out, N); return RGBL_OK; }
  const int words = (N + 63) / 64;
  std::vector<int32_t> feat((size_t)N), point((size_t)N);
  mlpnp_correspondences(in, feat.data(), point.data());
  MlView v;
  v.xy = in->kp_xy; v.oct = in->kp_octave; v.wpos = in->world_pos; v.sigma2 = in->level_sigma2; v.feat = feat.data(); v.point = point.data();
  v.N = N; v.n_levels = in->n_levels; v.th2 = in->th2;
  memcpy(v.K, in->K, sizeof(v.K));
  std::vector<MlpnpHypOut> hyp((size_t)in->n_hyp);
  std::vector<unsigned long long> mask((size_t)in->n_hyp * (size_t)words, 0ull), carried((size_t)words, 0ull);
  if (in->best_inliers > 0) mlpnp_mask_words(in->best_mask, N, carried.data());
  std::vector<MlWork> work(1);
  MlHostX x;
  auto check = [&](const double* R, const double* t, unsigned long long* m) {
    int count = 0;
    for (int w = 0; w < words; ++w) m[w] = 0ull;
    for (int i = 0; i < N; ++i)
      if (ml_is_inlier(v, R, t, i)) { m[i >> 6] |= 1ull << (i & 63); ++count; }
    return count;
  };
  for (int h = 0; h < in->n_hyp; ++h) {
    MlSixSums Q;
    const MlSet S = {&v, in->samples + 6 * (size_t)h, 6};
    MlpnpHypOut& o = hyp[(size_t)h];
    ml_compute_pose(x, work[0], Q, S, o.T, o.T + 9, &o.path);
    o.count = check(o.T, o.T + 9, mask.data() + (size_t)h * (size_t)words);
  }
  struct Counts {
    const MlpnpHypOut* h;
    int operator[](int k) const { return h[k].count; }
  };
  MlpnpResult r;
  memset(&r, 0, sizeof(r));
  r.scan = ml_scan(Counts{hyp.data()}, in->n_hyp, in->min_inliers, in->best_inliers);
  const MlScan& sc = r.scan;
  if (sc.record >= 0) ml_Tcw(hyp[(size_t)sc.record].T, hyp[(size_t)sc.record].T + 9, r.best_Tcw);
  else memcpy(r.best_Tcw, in->best_Tcw, sizeof(r.best_Tcw));
  if (sc.selected >= 0) ml_Tcw(hyp[(size_t)sc.selected].T, hyp[(size_t)sc.selected].T + 9, r.Tcw);
  else memcpy(r.Tcw, r.best_Tcw, sizeof(r.Tcw));
  std::vector<uint8_t> inl((size_t)N, 0), best((size_t)N, 0);
  const unsigned long long* bm = sc.record >= 0 ? mask.data() + (size_t)sc.record * (size_t)words : carried.data();
  const unsigned long long* om = sc.selected >= 0 ? mask.data() + (size_t)sc.selected * (size_t)words : bm;
  for (int i = 0; i < N; ++i) {
    best[(size_t)i] = (uint8_t)mask_bit(bm, i);
    inl[(size_t)i] = (uint8_t)mask_bit(om, i);
  }
  write_mlpnp_output(in, out, N, r, inl.data(), best.data(), hyp.data());
  return RGBL_OK;
}

int rgbl_mlpnp_ransac_batch(rgbl_matcher* m, int n_problems, const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out) {
  if (!m || n_problems < 0 || (n_problems > 0 && (!in || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int B = n_problems;
  if (B > 32767) { set_error("mlpnp: more than 32767 problems in one call"); return RGBL_ERR_INVALID; }
  PoolCall pc(m, "mlpnp", "the frame");
  BatchOffsets off(B);   // of the problems that run: hypotheses, mask words, correspondences; and the words of the carried-in masks
  std::vector<int> Ns((size_t)B, 0), cword_off((size_t)B + 1, 0);
  for (int b = 0; b < B; ++b) {
    RGBL_TRY(check_mlpnp_input(in + b, b, false, &Ns[(size_t)b]));
    RGBL_TRY(pc.note(in[b].pool, {in[b].device}, b));
    const bool run = !mlpnp_skipped(in + b, Ns[(size_t)b]);
    const int nh = run ? in[b].n_hyp : 0, nn = run ? Ns[(size_t)b] : 0;
    if (!off.add(b, nh, nn, 1, INT_MAX)) { set_error("mlpnp: more than 2^31 hypotheses in one call"); return RGBL_ERR_INVALID; }
    cword_off[(size_t)b + 1] = cword_off[(size_t)b] + (nn + 63) / 64;
  }
  if (off.word[(size_t)B] > (size_t)kMlMaxMaskWords) { set_error("mlpnp: more than 2^%d mask words (n_hyp x ceil(N / 64), all problems) in one call", kMlMaxMaskWordsLog2); return RGBL_ERR_INVALID; }
  const rgbl_map_points* pool = pc.pool;
  RGBL_TRY(pc.lock(B, [&](int b) -> int {
    for (int i = 0; in[b].pool && i < in[b].n_points; ++i)
      if (!pc.holds(in[b].slot[i])) { set_error("mlpnp %d: slot %d outside [0, %d)", b, in[b].slot[i], pool->cap); return RGBL_ERR_INVALID; }
    return RGBL_OK;
  }));
  const int H = off.hyp[(size_t)B], M = off.item[(size_t)B];
  if (H == 0) {   // nothing to run (B == 0 included)
    for (int b = 0; b < B; ++b) write_mlpnp_skipped(in + b, out + b, Ns[(size_t)b]);
    return RGBL_OK;
  }
  std::vector<int32_t> feat((size_t)M), point((size_t)M);
  std::vector<unsigned long long> carried((size_t)cword_off[(size_t)B], 0ull);
  for (int b = 0; b < B; ++b) {
    if (off.item[(size_t)b + 1] == off.item[(size_t)b]) continue;
    mlpnp_correspondences(in + b, feat.data() + off.item[(size_t)b], point.data() + off.item[(size_t)b]);
    if (in[b].best_inliers > 0) mlpnp_mask_words(in[b].best_mask, Ns[(size_t)b], carried.data() + cword_off[(size_t)b]);
  }
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);  // behind pc (PoolCall)
  HostCall hc(m);
  hipStream_t s = hc.s;
  std::vector<MlpnpProblem> prob((size_t)B);
  MlpnpDev D;
  memset(&D, 0, sizeof(D));
  bool diag = false;
  for (int b = 0; b < B; ++b) diag = diag || out[b].counts || out[b].Tcw_all || out[b].gn_path;
  RGBL_TRY(hc.begin([&]() -> int {
    const int32_t *d_feat = nullptr, *d_point = nullptr;
    const unsigned long long* d_carried = nullptr;
    hc.put(&d_feat, feat.data(), (size_t)M);
    hc.put(&d_point, point.data(), (size_t)M);
    hc.put(&d_carried, carried.data(), carried.size());
    for (int b = 0; b < B; ++b) {
      MlpnpProblem& P = prob[(size_t)b];
      memset(&P, 0, sizeof(P));
      const rgbl_mlpnp_input& I = in[b];
      if (mlpnp_skipped(&I, Ns[(size_t)b])) continue;   // n_hyp = 0: no workgroup touches it
      RGBL_TRY(put_features(hc, I.device, I.n, nullptr, I.kp_xy, I.kp_octave, nullptr, nullptr, &P.v.xy, &P.v.oct, nullptr));
      if (I.pool) P.v.wpos = pool->d_wpos; else hc.put(&P.v.wpos, I.world_pos, (size_t)I.n_points * 3);
      hc.put(&P.v.sigma2, I.level_sigma2, (size_t)I.n_levels);
      hc.put(&P.samples, I.samples, (size_t)I.n_hyp * 6);
      P.v.feat = d_feat + off.item[(size_t)b]; P.v.point = d_point + off.item[(size_t)b];
      P.v.N = Ns[(size_t)b]; P.v.n_levels = I.n_levels; P.v.th2 = I.th2;
      memcpy(P.v.K, I.K, sizeof(P.v.K));
      P.best_mask = I.best_inliers > 0 ? d_carried + cword_off[(size_t)b] : nullptr;
      P.n_hyp = I.n_hyp; P.min_inliers = I.min_inliers; P.best_inliers = I.best_inliers;
      P.hyp_off = off.hyp[(size_t)b]; P.word_off = (int)off.word[(size_t)b]; P.words = (Ns[(size_t)b] + 63) / 64;
      P.corr_off = off.item[(size_t)b]; P.cword_off = cword_off[(size_t)b];
      memcpy(P.best_Tcw, I.best_Tcw, sizeof(P.best_Tcw));
    }
    D.prob = hc.stage<MlpnpProblem>((size_t)B, [&](MlpnpProblem* dst) { memcpy(dst, prob.data(), sizeof(MlpnpProblem) * (size_t)B); });
    D.res = hc.result<MlpnpResult>((size_t)B);   // what comes back, side by side
    D.inlier = hc.result<uint8_t>((size_t)M);
    D.best_out = hc.result<uint8_t>((size_t)M);
    D.hyp = diag ? hc.result<MlpnpHypOut>((size_t)H) : hc.scratch<MlpnpHypOut>((size_t)H);
    D.mask = hc.scratch<unsigned long long>(off.word[(size_t)B]);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_mlpnp_hypotheses", k_mlpnp_hypotheses, dim3((unsigned)((off.max_hyp + kMlHypPerGroup - 1) / kMlHypPerGroup), (unsigned)B), dim3(256), 0, D));
  RGBL_TRY(launch(m, s, "k_mlpnp_select", k_mlpnp_select, dim3((unsigned)B), dim3(256), 0, D));
  RGBL_TRY(hc.fetch());
  for (int b = 0; b < B; ++b) {
    if (mlpnp_skipped(in + b, Ns[(size_t)b])) { write_mlpnp_skipped(in + b, out + b, Ns[(size_t)b]); continue; }
    write_mlpnp_output(in + b, out + b, Ns[(size_t)b], hc.host(D.res)[b], hc.host(D.inlier) + off.item[(size_t)b], hc.host(D.best_out) + off.item[(size_t)b],
                       diag ? hc.host(D.hyp) + off.hyp[(size_t)b] : nullptr);
  }
  return RGBL_OK;
}

int rgbl_mlpnp_ransac(rgbl_matcher* m, const rgbl_mlpnp_input* in, rgbl_mlpnp_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return rgbl_mlpnp_ransac_batch(m, 1, in, out);
}

// ---- TwoViewReconstruction (src/TwoViewReconstruction.cc) -------------------------------------------------------------------
namespace {
constexpr int kTvMaxHyp = 1 << 20;
constexpr int kTvMaxMaskWordsLog2 = 26;   // 512 MB of masks
constexpr size_t kTvMaxMaskWords = (size_t)1 << kTvMaxMaskWordsLog2;
constexpr int kTvMaxKeysLog2 = 24;           // keys of frame 1 over the problems of a call that run: 104 B of CheckRT scratch each, 1.7 GB
constexpr size_t kTvMaxKeys = (size_t)1 << kTvMaxKeysLog2;
// Everything that can be refused is refused here, before anything is staged, launched or written.  *n_match = N.
int check_two_view_input(const rgbl_two_view_input* in, int b, bool host_only, int* n_match) {
  *n_match = 0;
  if (in->n1 < 0 || in->n1 > 65535 || in->n2 < 0 || in->n2 > 65535) { set_error("two view %d: n1 or n2 outside [0, 65535]", b); return RGBL_ERR_INVALID; }
  if (in->n_hyp < 0 || in->n_hyp > kTvMaxHyp) { set_error("two view %d: n_hyp outside [0, %d]", b, kTvMaxHyp); return RGBL_ERR_INVALID; }
  bool finite = std::isfinite(in->sigma);
  for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(in->K[i]);
  if (!finite) { set_error("two view %d: K or sigma is not finite", b); return RGBL_ERR_INVALID; }
  if (host_only && (in->device1 || in->device2)) { set_error("two view %d: the host build reads host arrays only", b); return RGBL_ERR_INVALID; }
  if (in->device1 ? in->device1->n != in->n1 : (in->n1 > 0 && !in->kp1_xy)) { set_error("two view %d: frame 1 is either kp1_xy or a resident frame of n1 features", b); return RGBL_ERR_INVALID; }
  if (in->device2 ? in->device2->n != in->n2 : (in->n2 > 0 && !in->kp2_xy)) { set_error("two view %d: frame 2 is either kp2_xy or a resident frame of n2 features", b); return RGBL_ERR_INVALID; }
  if (in->n1 > 0 && !in->matches12) { set_error("two view %d: no matches12", b); return RGBL_ERR_INVALID; }
  int N = 0;
  for (int i = 0; i < in->n1; ++i) {
    const int q = in->matches12[i];
    if (q < -1 || q >= in->n2) { set_error("two view %d: matches12[%d] = %d outside [-1, %d)", b, i, q, in->n2); return RGBL_ERR_INVALID; }
    N += q >= 0 ? 1 : 0;
  }
  if (in->n_hyp > 0) {
    if (N < 8) { set_error("two view %d: %d matches, a set needs 8", b, N); return RGBL_ERR_INVALID; }
    if (!in->samples) { set_error("two view %d: no samples", b); return RGBL_ERR_INVALID; }
    for (int k = 0; k < in->n_hyp; ++k) {
      if (!distinct_in_range(in->samples + 8 * (size_t)k, 8, N)) { set_error("two view %d: set %d is not eight distinct indices in [0, %d)", b, k, N); return RGBL_ERR_INVALID; }
    }
  }
  *n_match = N;
  return RGBL_OK;
}
// mvMatches12 (:55-64)
void two_view_matches(const rgbl_two_view_input* in, int32_t* m1, int32_t* m2) {
  int k = 0;
  for (int i = 0; i < in->n1; ++i)
    if (in->matches12[i] >= 0) { m1[k] = i; m2[k] = in->matches12[i]; ++k; }
}
// n_hyp == 0: both scores stay 0 (:144, :195), the exit of :113
void write_two_view_skipped(rgbl_two_view_output* out) {
  out->found = 0; out->model = -1; out->exit_code = kTvNoScore; out->SH = 0.0f; out->SF = 0.0f; out->best_h = -1; out->best_f = -1;
  for (int k = 0; k < 9; ++k) { out->H21[k] = 0.0f; out->F21[k] = 0.0f; out->R21[k] = (k % 4 == 0) ? 1.0f : 0.0f; }
  for (int k = 0; k < 3; ++k) out->t21[k] = 0.0f;
  out->p3d_assigned = 0; out->n_inliers = 0; out->best_motion = -1; out->aux = 0;
  for (int k = 0; k < 8; ++k) { out->n_good[k] = 0; out->parallax[k] = 0.0f; }
}
// p3d / tri: the winning hypothesis's, per key of frame 1; mask_h / mask_f: per match; score / model: per hypothesis (null: not fetched)
void write_two_view_output(const rgbl_two_view_input* in, rgbl_two_view_output* out, int N, const TvResult& r, const float* p3d, const uint8_t* tri,
                           const uint8_t* mask_h, const uint8_t* mask_f, const float* score, const float* model) {
  out->found = r.found; out->model = r.model; out->exit_code = r.exit_code; out->SH = r.SH; out->SF = r.SF; out->best_h = r.best_h; out->best_f = r.best_f;
  memcpy(out->H21, r.H21, sizeof(out->H21));
  memcpy(out->F21, r.F21, sizeof(out->F21));
  memcpy(out->R21, r.R, sizeof(out->R21));
  memcpy(out->t21, r.t, sizeof(out->t21));
  if (r.found && out->p3d) memcpy(out->p3d, p3d, sizeof(float) * 3 * (size_t)in->n1);
  if (r.found && out->triangulated) memcpy(out->triangulated, tri, (size_t)in->n1);
  out->p3d_assigned = r.found && r.model == 1 ? 1 : 0;
  out->n_inliers = r.n_inliers; out->best_motion = r.best; out->aux = r.aux;
  memcpy(out->n_good, r.n_good, sizeof(out->n_good));
  memcpy(out->parallax, r.parallax, sizeof(out->parallax));
  if (out->inliers_h) memcpy(out->inliers_h, mask_h, (size_t)N);
  if (out->inliers_f && r.best_f >= 0) memcpy(out->inliers_f, mask_f, (size_t)N);
  if (out->scores && score) memcpy(out->scores, score, sizeof(float) * 2 * (size_t)in->n_hyp);
  if (out->models && model) memcpy(out->models, model, sizeof(float) * 18 * (size_t)in->n_hyp);
}
}  // namespace

int rgbl_two_view_reconstruct_host(const rgbl_two_view_input* in, rgbl_two_view_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  int N = 0;
  RGBL_TRY(check_two_view_input(in, 0, true, &N));
  if (in->n_hyp == 0) { write_two_view_skipped(out); return RGBL_OK; }
  const int words = (N + 63) / 64, n1 = in->n1, H = in->n_hyp;
  std::vector<int32_t> m1((size_t)N), m2((size_t)N);
  two_view_matches(in, m1.data(), m2.data());
  TvView v;
  v.xy1 = in->kp1_xy; v.xy2 = in->kp2_xy; v.m1 = m1.data(); v.m2 = m2.data(); v.N = N; v.n1 = n1; v.n2 = in->n2; v.sigma = in->sigma;
  memcpy(v.K, in->K, sizeof(v.K));
  TvHostX x;
  float buf[2][64];
  tv_normalize(x, buf, v.xy1, v.n1, v.T1);
  tv_normalize(x, buf, v.xy2, v.n2, v.T2);
  std::vector<TvWork> work(1);
  std::vector<float> score(2 * (size_t)H), model(18 * (size_t)H);
  std::vector<unsigned long long> mask(2 * (size_t)H * (size_t)words, 0ull);
  const float invSigmaSquare = tv_inv_sigma2(v.sigma);
  for (int h = 0; h < H; ++h)
    for (int md = 0; md < 2; ++md) {
      float M[9], M2[9];
      tv_model(x, work[0], v, in->samples + 8 * (size_t)h, md, M, M2);
      unsigned long long* mk = mask.data() + (2 * (size_t)h + (size_t)md) * (size_t)words;
      float sc = 0.0f;
      for (int i = 0; i < N; ++i) {
        float t[2];
        if (tv_check(md, M, M2, v, i, invSigmaSquare, t)) mk[i >> 6] |= 1ull << (i & 63);
        sc = tv_add_chunk(sc, t, 2);
      }
      score[2 * (size_t)h + md] = sc;
      memcpy(model.data() + 9 * (2 * (size_t)h + md), M, sizeof(M));
    }
  TvResult r;
  memset(&r, 0, sizeof(r));
  r.best_h = tv_first_max(score.data(), H, 0, &r.SH);
  r.best_f = tv_first_max(score.data(), H, 1, &r.SF);
  r.model = tv_choose_model(r.SH, r.SF);
  if (r.best_h >= 0) memcpy(r.H21, model.data() + 9 * (2 * (size_t)r.best_h), sizeof(r.H21));
  if (r.best_f >= 0) memcpy(r.F21, model.data() + 9 * (2 * (size_t)r.best_f + 1), sizeof(r.F21));
  std::vector<uint8_t> mask_h((size_t)N, 0), mask_f((size_t)N, 0);
  const unsigned long long* mh = r.best_h >= 0 ? mask.data() + (2 * (size_t)r.best_h) * (size_t)words : nullptr;
  const unsigned long long* mf = r.best_f >= 0 ? mask.data() + (2 * (size_t)r.best_f + 1) * (size_t)words : nullptr;
  for (int i = 0; i < N; ++i) {
    mask_h[(size_t)i] = mh ? (uint8_t)mask_bit(mh, i) : (uint8_t)0;
    mask_f[(size_t)i] = mf ? (uint8_t)mask_bit(mf, i) : (uint8_t)0;
  }
  TvMotions mo;
  mo.n = 0;
  TvDecision d = {0, kTvFound, -1, 0};
  const uint8_t* chosen = nullptr;
  if (r.model < 0) d.exit_code = kTvNoScore;
  else if (r.model == 0) { chosen = mask_h.data(); if (!tv_motions_h(r.H21, v.K, mo)) d.exit_code = kTvHRatio; }
  else { chosen = mask_f.data(); tv_motions_f(r.F21, v.K, mo); }
  for (int i = 0; chosen && i < N; ++i) r.n_inliers += chosen[i];
  std::vector<float> p3d(3 * (size_t)n1 * kTvMaxMotions, 0.0f);
  std::vector<uint8_t> good((size_t)n1 * kTvMaxMotions, 0);
  for (int j = 0; j < mo.n; ++j) {
    TvCam c;
    tv_cam(v.K, mo.R[j], mo.t[j], v.sigma, c);
    float* P = p3d.data() + 3 * (size_t)j * (size_t)n1;
    uint8_t* G = good.data() + (size_t)j * (size_t)n1;
    std::vector<float> cosv;   // the values that take part in the order (a NaN does not)
    int nGood = 0;
    for (int i = 0; i < N; ++i) {
      if (!chosen[i]) continue;
      const size_t a = (size_t)m1[(size_t)i], q = (size_t)m2[(size_t)i];
      float p[3], cp;
      const int code = tv_rt_point(c, v.xy1[2 * a], v.xy1[2 * a + 1], v.xy2[2 * q], v.xy2[2 * q + 1], p, &cp);
      if (!code) continue;
      P[3 * a] = p[0]; P[3 * a + 1] = p[1]; P[3 * a + 2] = p[2];
      G[a] = code == 2 ? 1 : 0;
      if (cp == cp) cosv.push_back(cp);
      ++nGood;
    }
    r.n_good[j] = nGood;
    if (nGood > 0) {
      std::sort(cosv.begin(), cosv.end());
      const size_t idx = (size_t)std::min(50, nGood - 1);
      r.parallax[j] = tv_parallax_deg(idx < cosv.size() ? cosv[idx] : np_float(0x7fc00000u));
    }
  }
  if (d.exit_code == kTvFound) d = r.model == 0 ? tv_decide_h(r.n_good, r.parallax, r.n_inliers) : tv_decide_f(r.n_good, r.parallax, r.n_inliers);
  r.found = d.found; r.exit_code = d.exit_code; r.best = d.best; r.aux = d.aux;
  for (int k = 0; k < 9; ++k) r.R[k] = d.found ? mo.R[d.best][k] : ((k % 4 == 0) ? 1.0f : 0.0f);
  for (int k = 0; k < 3; ++k) r.t[k] = d.found ? mo.t[d.best][k] : 0.0f;
  const size_t w = d.found ? (size_t)d.best : 0;
  write_two_view_output(in, out, N, r, p3d.data() + 3 * w * (size_t)n1, good.data() + w * (size_t)n1, mask_h.data(), mask_f.data(), score.data(), model.data());
  return RGBL_OK;
}

int rgbl_two_view_reconstruct_batch(rgbl_matcher* m, int n_problems, const rgbl_two_view_input* in, rgbl_two_view_output* out) {
  if (!m || n_problems < 0 || (n_problems > 0 && (!in || !out))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int B = n_problems;
  if (B > 32767) { set_error("two view: more than 32767 problems in one call"); return RGBL_ERR_INVALID; }
  PoolCall pc(m, "two view", "a frame");
  BatchOffsets off(B);   // of the problems that run: hypotheses, mask words (two masks each), matches; and the keys of frame 1
  std::vector<int> Ns((size_t)B, 0);
  std::vector<size_t> key_off((size_t)B + 1, 0);
  for (int b = 0; b < B; ++b) {
    RGBL_TRY(check_two_view_input(in + b, b, false, &Ns[(size_t)b]));
    RGBL_TRY(pc.note(nullptr, {in[b].device1, in[b].device2}, b));
    const bool run = in[b].n_hyp > 0;
    const int nh = run ? in[b].n_hyp : 0, nn = run ? Ns[(size_t)b] : 0;
    if (!off.add(b, nh, nn, 2, INT_MAX / 2)) { set_error("two view: more than 2^30 hypotheses in one call"); return RGBL_ERR_INVALID; }
    key_off[(size_t)b + 1] = key_off[(size_t)b] + (size_t)(run ? in[b].n1 : 0);   // at most 65535 each: B < 2^15 problems fit an int
  }
  if (off.word[(size_t)B] > kTvMaxMaskWords) { set_error("two view: more than 2^%d mask words (2 x n_hyp x ceil(N / 64), all problems) in one call", kTvMaxMaskWordsLog2); return RGBL_ERR_INVALID; }
  if (key_off[(size_t)B] > kTvMaxKeys) { set_error("two view: more than 2^%d keys of frame 1 (all problems with n_hyp > 0) in one call", kTvMaxKeysLog2); return RGBL_ERR_INVALID; }
  const int H = off.hyp[(size_t)B];
  const size_t M = off.item[(size_t)B], Kn = key_off[(size_t)B];
  if (H == 0) {   // nothing to run (B == 0 included)
    for (int b = 0; b < B; ++b) write_two_view_skipped(out + b);
    return RGBL_OK;
  }
  std::vector<int32_t> m1(M), m2(M);
  for (int b = 0; b < B; ++b)
    if (in[b].n_hyp > 0) two_view_matches(in + b, m1.data() + off.item[(size_t)b], m2.data() + off.item[(size_t)b]);
  RGBL_HIP(hipSetDevice(m->device));
  StreamDrain drain(m->stream);
  HostCall hc(m);
  hipStream_t s = hc.s;
  std::vector<TvProblem> prob((size_t)B);
  TvDev D;
  memset(&D, 0, sizeof(D));
  bool diag = false;
  for (int b = 0; b < B; ++b) diag = diag || out[b].scores || out[b].models;
  RGBL_TRY(hc.begin([&]() -> int {
    const int32_t *d_m1 = nullptr, *d_m2 = nullptr;
    hc.put(&d_m1, m1.data(), M);
    hc.put(&d_m2, m2.data(), M);
    for (int b = 0; b < B; ++b) {
      TvProblem& P = prob[(size_t)b];
      memset(&P, 0, sizeof(P));
      const rgbl_two_view_input& I = in[b];
      if (I.n_hyp == 0) continue;   // no workgroup touches it
      RGBL_TRY(put_features(hc, I.device1, I.n1, nullptr, I.kp1_xy, nullptr, nullptr, nullptr, &P.v.xy1, nullptr, nullptr));
      RGBL_TRY(put_features(hc, I.device2, I.n2, nullptr, I.kp2_xy, nullptr, nullptr, nullptr, &P.v.xy2, nullptr, nullptr));
      hc.put(&P.samples, I.samples, (size_t)I.n_hyp * 8);
      P.v.m1 = d_m1 + off.item[(size_t)b]; P.v.m2 = d_m2 + off.item[(size_t)b];
      P.v.N = Ns[(size_t)b]; P.v.n1 = I.n1; P.v.n2 = I.n2; P.v.sigma = I.sigma;
      memcpy(P.v.K, I.K, sizeof(P.v.K));
      P.n_hyp = I.n_hyp; P.words = (Ns[(size_t)b] + 63) / 64; P.hyp_off = off.hyp[(size_t)b];
      P.match_off = (int)off.item[(size_t)b]; P.key_off = (int)key_off[(size_t)b]; P.word_off = (unsigned long long)off.word[(size_t)b];
    }
    D.prob = hc.stage<TvProblem>((size_t)B, [&](TvProblem* dst) { memcpy(dst, prob.data(), sizeof(TvProblem) * (size_t)B); });
    D.res = hc.result<TvResult>((size_t)B);   // what comes back, side by side
    D.p3d_out = hc.result<float>(3 * Kn);
    D.tri_out = hc.result<uint8_t>(Kn);
    D.mask_h = hc.result<uint8_t>(M);
    D.mask_f = hc.result<uint8_t>(M);
    D.score = diag ? hc.result<float>(2 * (size_t)H) : hc.scratch<float>(2 * (size_t)H);
    D.model = diag ? hc.result<float>(18 * (size_t)H) : hc.scratch<float>(18 * (size_t)H);
    D.norm = hc.scratch<float>(8 * (size_t)B);
    D.mask = hc.scratch<unsigned long long>(off.word[(size_t)B]);
    D.sel = hc.scratch<TvSelect>((size_t)B);
    D.n_good = hc.scratch<int32_t>(8 * (size_t)B);
    D.parallax = hc.scratch<float>(8 * (size_t)B);
    D.cosv = hc.scratch<float>(8 * M);
    D.p3d = hc.scratch<float>(24 * Kn);
    D.good = hc.scratch<uint8_t>(8 * Kn);
    return RGBL_OK;
  }));
  RGBL_TRY(launch(m, s, "k_tv_normalize", k_tv_normalize, dim3(2, (unsigned)B), dim3(64), 0, D));
  RGBL_TRY(launch(m, s, "k_tv_hypotheses", k_tv_hypotheses, dim3((unsigned)((off.max_hyp + kTvHypPerGroup - 1) / kTvHypPerGroup), 2, (unsigned)B), dim3(256), 0, D));
  RGBL_TRY(launch(m, s, "k_tv_select", k_tv_select, dim3((unsigned)B), dim3(256), 0, D));
  RGBL_TRY(launch(m, s, "k_tv_check_rt", k_tv_check_rt, dim3(kTvMaxMotions, (unsigned)B), dim3(256), 0, D));
  RGBL_TRY(launch(m, s, "k_tv_decide", k_tv_decide, dim3((unsigned)B), dim3(256), 0, D));
  RGBL_TRY(hc.fetch());
  for (int b = 0; b < B; ++b) {
    if (in[b].n_hyp == 0) { write_two_view_skipped(out + b); continue; }
    write_two_view_output(in + b, out + b, Ns[(size_t)b], hc.host(D.res)[b], hc.host(D.p3d_out) + 3 * key_off[(size_t)b], hc.host(D.tri_out) + key_off[(size_t)b],
                          hc.host(D.mask_h) + off.item[(size_t)b], hc.host(D.mask_f) + off.item[(size_t)b],
                          diag ? hc.host(D.score) + 2 * (size_t)off.hyp[(size_t)b] : nullptr, diag ? hc.host(D.model) + 18 * (size_t)off.hyp[(size_t)b] : nullptr);
  }
  return RGBL_OK;
}

int rgbl_two_view_reconstruct(rgbl_matcher* m, const rgbl_two_view_input* in, rgbl_two_view_output* out) {
  if (!in || !out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  return rgbl_two_view_reconstruct_batch(m, 1, in, out);
}

}  // extern "C"
