// lba_math.h — Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1188-1497) for single-camera pinhole key frames with
// monocular and stereo / RGB-L edges mixed, in ONE place for host and device: the two binary edges with their analytic
// Jacobians, Huber, g2o's block solver with the Schur complement, its Levenberg and the final flags, restated from
//   src/Optimizer.cc, src/OptimizableTypes.cpp:139 (EdgeSE3ProjectXYZ), src/CameraModels/Pinhole.cpp        (the reference)
//   Thirdparty/g2o/g2o/core/{block_solver.hpp,base_binary_edge.hpp,optimization_algorithm_levenberg.cpp,sparse_optimizer.cpp},
//   types/types_six_dof_expmap.cpp:228 (EdgeStereoSE3ProjectXYZ), types/{se3quat.h,types_sba.h}                (its g2o)
// The rig edge (:1366-1400), KannalaBrandt8 and LocalInertialBA have no form here.
//
// Every step is a function of ONE item (an edge, a point, a camera's lane, a lane of a Schur block) over an LbaView of plain
// arrays: the kernels of csrc/lba.hip call it with the item a work-item owns, the host build calls it in a loop.  All arithmetic
// is fp64, no contraction; sin / cos, SE3Quat and Huber are csrc/poseopt_math.h's.
//
// Edge k is the k-th edge the reference creates (point-major).  A camera is ACTIVE when it is free, not flagged fixed and has
// an edge; the active cameras, in list order, are the columns 0 .. nA-1 of the reduced system (n = 6 nA).  A point is active
// when it has an edge.  The unknowns are numbered cameras first (6 per column), then the active points in order (3 each).
//
// Summation orders (host, emulator and GPU agree bit for bit; no floating-point atomics):
//   per point p         Hll_p and b_p over p's edges in ascending k, serially, from zero
//   per active camera   Hpp_c (upper triangle, 21) and b_c (6): the j-th edge of the camera's list (ascending k) belongs to
//                       lane j mod 64, a lane adds its edges in ascending j, and the 64 partial sums are combined by
//                       lm_math.h's tree v[i] = v[i] + v[i + s], s = 32, 16, ..., 1
//   Schur complement    g2o's association (block_solver.hpp:383-433): Dinv = (Hll_p + lambda I)^-1 by the cofactor formula,
//                       BDinv = B_i Dinv, S_ij -= BDinv B_j^T for j >= i, coeff_i += B_i (Dinv b_p), b_schur = b - coeff.  A
//                       diagonal block starts as Hpp_i + lambda I, the others as zero; the contributions to a block arrive
//                       in ascending point order, each one a three-term product subtracted as a whole.  The upper triangle
//                       of S is what the solver reads (a diagonal block's lower half is not formed).
//   reduced solve       lm_solve_n of lm_math.h: LDL^T without pivoting, every element a - sum_p (L_ip L_jp) D_p with p
//                       ascending.  The reference's SimplicialLDLT with AMD ordering is not pinned.
//   back-substitution   x_p = Dinv (b_p - sum_e B_e^T x_cam(e)), e ascending, each B_e^T x a six-term sum left to right
//   whole-system sums   the robust chi2 over edge index and computeScale's sum over unknown index: lm_math.h's 256 lanes
//                       (item k on lane k mod 256, ascending, the tree s = 128 .. 1).  computeLambdaInit's maximum takes the
//                       same lanes and tree with std::max(a, m) = (a < m) ? m : a, so a NaN diagonal gives the same lambda
//                       everywhere (in g2o it depends on the vertex order).
//
// Levenberg's scalar control is lm_levenberg_loop of lm_math.h, the solve and the passes behind a policy, the stop
// flag polled exactly where g2o polls it, computeLambdaInit over ALL active vertices and user_lambda_init.  The quirks listed
// at the top of lm_math.h hold: a failed factorisation gives tempChi = DBL_MAX, x (cameras AND points) persists across failed
// factorisations, and the edges keep the chi2 of the last TRIED step.  Edges whose error was never computed (max_iterations
// < 1, or a stop before the first iteration) hold uninitialised memory in g2o; here their chi2 is 0.
#pragma once
#include "poseopt_math.h"

namespace rgbl {

constexpr int kLbaCamLanes = 64;         // lanes of one camera's diagonal block
constexpr int kLbaSchurLanes = 64;       // work-items of one Schur block: 36 entries, 6 rows of coeff
constexpr int kLbaMaxFree = 128;         // the reduced system is dense: 768^2 doubles
constexpr int kLbaMaxFixed = 1024;
constexpr int kLbaMaxPoints = 1 << 18;
constexpr int kLbaMaxEdges = 1 << 20;
constexpr int kLbaLdsCams = 20;          // the factorisation keeps the triangle in LDS up to n = 120 (58 080 bytes, next to 3 x 768 doubles of vectors)
constexpr int kLbaLdsN = 6 * kLbaLdsCams;

struct LbaEdgeLin { double Hpp[21], bc[6], W[18], Hll[6], bp[3]; };   // W = Hpl's block, 6 x 3 row-major: B^T (rho1 Omega) A
struct LbaEdgeTrial { double BD[18], Bdb[6]; };                       // W Dinv and W (Dinv b_p) of the trial's lambda
struct LbaRecord { double chi, maxdiag, scale; int32_t ok, reserved; };

struct LbaView {
  int nC, nA, nP, nE, nPa, n;
  int robust;                      // 1: every edge has its Huber kernel (LocalBundleAdjustment); 0: none (BundleAdjustment's bRobust)
  double delta[2];                 // Huber's delta of a monocular and of a stereo edge, as the float the caller's reference sets:
                                   // sqrt(5.991), sqrt(7.815) (LocalBundleAdjustment, :1275-1276); sqrt(5.99), sqrt(7.815) (BundleAdjustment, :131-132)
  PoPose* T; PoPose* Tt;           // the cameras' estimates and the trial's (free ++ fixed)
  const PoCam* C;
  const int32_t* col;              // camera -> column, -1: fixed or without an edge
  const int32_t* col_cam;          // column -> camera
  double* X; double* Xt;           // the points' estimates and the trial's
  const int32_t* pt_off;           // nP + 1: point p owns the edges pt_off[p] .. pt_off[p + 1]
  const int32_t* act_pt;           // nPa: the active points in order
  const int32_t* e_pt; const int32_t* e_cam;
  const float* e_obs;              // 3 per edge, obs[2] < 0: monocular
  const float* e_info;
  double* e_chi2; double* e_rho;   // chi2 of the error computed last, and its Huber rho[0]
  LbaEdgeLin* lin; LbaEdgeTrial* tr;
  const int32_t* cam_eoff;         // nA + 1: column a owns cam_edges[cam_eoff[a] .. cam_eoff[a + 1]], ascending k
  const int32_t* cam_edges;
  const int32_t* blk_off;          // nA (nA + 1) / 2 + 1: the (edge of column i, edge of column j) pairs of the upper block (i, j)
  const int32_t* pairs;            // 2 per pair, ascending point order
  double* pt_H; double* pt_b;      // 6 + 3 per point
  double* cam_H; double* cam_b;    // 21 + 6 per column
  double* S;                       // the reduced matrix, lm_solve_n's layout
  double* bs; double* x_cam;       // n each
  double* x_pt;                    // 3 per point
  LbaRecord* rec;
  uint8_t* flags;
  // BundleAdjustment's panel solve (csrc/gba.hip; unused by LocalBundleAdjustment)
  const int32_t* blk_list; int n_blk_list;   // 2 per upper block that is not empty: (i, j)
  double* pD; double* py; double* pyf;       // n each: the pivots, the forward sweep's running and final values
  double* pxw;                               // n: the backward sweep's running values
  int32_t* pfail;                            // 1: a pivot failed; every later kernel of the solve leaves at once
};

RGBL_HD bool lba_stereo(const float* obs) { return !(obs[2] < 0.0f); }   // :1305 / :1332
RGBL_HD int lba_block(int nA, int i, int j) { return i * nA - i * (i - 1) / 2 + (j - i); }   // upper block (i, j), i <= j

// computeError() and chi2() of EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ: po_edge_error with the point a vertex
RGBL_HD double lba_edge_error(const float* obs, double s, bool stereo, const PoCam& C, const PoPose& T, const double X[3],
                              double P[3], double err[3]) {
  po_map(T, X, P);
  if (stereo) {   // cam_project (types_six_dof_expmap.cpp:189-196): invz is a FLOAT
    const double invz = (double)(float)(1.0 / P[2]);
    const double u = P[0] * invz * C.fx + C.cx, v = P[1] * invz * C.fy + C.cy;
    err[0] = (double)obs[0] - u;
    err[1] = (double)obs[1] - v;
    err[2] = (double)obs[2] - (u - C.bf * invz);
    const double w0 = (s * err[0] + 0.0 * err[1]) + 0.0 * err[2], w1 = (0.0 * err[0] + s * err[1]) + 0.0 * err[2],
                 w2 = (0.0 * err[0] + 0.0 * err[1]) + s * err[2];
    return (err[0] * w0 + err[1] * w1) + err[2] * w2;
  }
  err[0] = (double)obs[0] - (C.fx * P[0] / P[2] + C.cx);   // Pinhole::project (Pinhole.cpp:35-41)
  err[1] = (double)obs[1] - (C.fy * P[1] / P[2] + C.cy);
  err[2] = 0.0;
  const double w0 = s * err[0] + 0.0 * err[1], w1 = 0.0 * err[0] + s * err[1];
  return err[0] * w0 + err[1] * w1;
}

// Quaterniond::toRotationMatrix as Eigen writes it, row-major
RGBL_HD void lba_rotation(const double q[4], double R[9]) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0],
               tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// rho[0] and rho[1] of an edge: Huber with the edge's delta, or - an edge without a kernel (constructQuadraticForm's plain
// branch, base_binary_edge.hpp:94-113; SparseOptimizer::activeRobustChi2 adds chi2 itself) - rho = (chi2, 1, 0)
RGBL_HD void lba_rho(const LbaView& V, double chi2, bool stereo, double* rho0, double* rho1) {
  if (V.robust) { po_huber(chi2, V.delta[stereo ? 1 : 0], rho0, rho1); return; }
  *rho0 = chi2;
  *rho1 = 1.0;
}

// the chi2 of edge k at the estimates (T, X) of every camera and point, kept with the edge
RGBL_HD void lba_edge_chi2(const LbaView& V, int k, const PoPose* T, const double* X) {
  const int p = V.e_pt[k], c = V.e_cam[k];
  const float* obs = V.e_obs + 3 * (size_t)k;
  const bool stereo = lba_stereo(obs);
  double P[3], err[3], r0, r1;
  const double chi2 = lba_edge_error(obs, (double)V.e_info[k], stereo, V.C[c], T[c], X + 3 * (size_t)p, P, err);
  lba_rho(V, chi2, stereo, &r0, &r1);
  V.e_chi2[k] = chi2;
  V.e_rho[k] = r0;
}

// linearizeOplus and constructQuadraticForm (base_binary_edge.hpp:56-115, the robust branch) of edge k at the current
// estimates: the edge's blocks go to V.lin[k].  A fixed camera contributes no block (Hpp, bc and W are left alone).
RGBL_HD void lba_linearise_edge(const LbaView& V, int k) {
  const int p = V.e_pt[k], c = V.e_cam[k];
  const float* obs = V.e_obs + 3 * (size_t)k;
  const bool stereo = lba_stereo(obs);
  const PoCam& C = V.C[c];
  const PoPose& T = V.T[c];
  const double s = (double)V.e_info[k];
  double P[3], err[3], rho0, rho1, R[9], A[3][3], B[3][6];
  const double chi2 = lba_edge_error(obs, s, stereo, C, T, V.X + 3 * (size_t)p, P, err);
  lba_rho(V, chi2, stereo, &rho0, &rho1);
  V.e_chi2[k] = chi2;
  V.e_rho[k] = rho0;
  lba_rotation(T.q, R);
  const double x = P[0], y = P[1], z = P[2];
  if (stereo) {   // types_six_dof_expmap.cpp:228-275
    const double z_2 = z * z, fx = C.fx, fy = C.fy, bf = C.bf;
    for (int j = 0; j < 3; ++j) {
      A[0][j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
      A[1][j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
      A[2][j] = A[0][j] - bf * R[6 + j] / z_2;
    }
    B[0][0] = x * y / z_2 * fx;
    B[0][1] = -(1.0 + (x * x / z_2)) * fx;
    B[0][2] = y / z * fx;
    B[0][3] = -1.0 / z * fx;
    B[0][4] = 0.0;
    B[0][5] = x / z_2 * fx;
    B[1][0] = (1.0 + y * y / z_2) * fy;
    B[1][1] = -x * y / z_2 * fy;
    B[1][2] = -x / z * fy;
    B[1][3] = 0.0;
    B[1][4] = -1.0 / z * fy;
    B[1][5] = y / z_2 * fy;
    B[2][0] = B[0][0] - bf * y / z_2;
    B[2][1] = B[0][1] + bf * x / z_2;
    B[2][2] = B[0][2];
    B[2][3] = B[0][3];
    B[2][4] = 0.0;
    B[2][5] = B[0][5] - bf / z_2;
  } else {        // OptimizableTypes.cpp:139-161 with Pinhole::projectJac (Pinhole.cpp:71-81): the full products
    const double J[2][3] = {{-(C.fx / z), -0.0, -(-C.fx * x / (z * z))}, {-0.0, -(C.fy / z), -(-C.fy * y / (z * z))}};
    const double D[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    for (int r = 0; r < 2; ++r) {
      for (int j = 0; j < 3; ++j) A[r][j] = (J[r][0] * R[j] + J[r][1] * R[3 + j]) + J[r][2] * R[6 + j];
      for (int j = 0; j < 6; ++j) B[r][j] = (J[r][0] * D[0][j] + J[r][1] * D[1][j]) + J[r][2] * D[2][j];
    }
    for (int j = 0; j < 3; ++j) A[2][j] = 0.0;
    for (int j = 0; j < 6; ++j) B[2][j] = 0.0;
  }
  const int rows = stereo ? 3 : 2;
  const double w = rho1 * s;                                                             // robustInformation: rho[1] * information
  const double o[3] = {-(s * err[0]) * rho1, -(s * err[1]) * rho1, -(s * err[2]) * rho1};   // omega_r = -omega * _error; *= rho[1]
  LbaEdgeLin& L = V.lin[k];
  int q = 0;
  for (int i = 0; i < 3; ++i) {
    for (int j = i; j < 3; ++j, ++q) {
      double h = A[0][i] * (w * A[0][j]) + A[1][i] * (w * A[1][j]);
      if (rows == 3) h = h + A[2][i] * (w * A[2][j]);
      L.Hll[q] = h;
    }
    double g = A[0][i] * o[0] + A[1][i] * o[1];
    if (rows == 3) g = g + A[2][i] * o[2];
    L.bp[i] = g;
  }
  if (V.col[c] < 0) return;
  q = 0;
  for (int i = 0; i < 6; ++i) {
    for (int j = i; j < 6; ++j, ++q) {
      double h = B[0][i] * (w * B[0][j]) + B[1][i] * (w * B[1][j]);
      if (rows == 3) h = h + B[2][i] * (w * B[2][j]);
      L.Hpp[q] = h;
    }
    for (int j = 0; j < 3; ++j) {
      double h = B[0][i] * (w * A[0][j]) + B[1][i] * (w * A[1][j]);
      if (rows == 3) h = h + B[2][i] * (w * A[2][j]);
      L.W[3 * i + j] = h;
    }
    double g = B[0][i] * o[0] + B[1][i] * o[1];
    if (rows == 3) g = g + B[2][i] * o[2];
    L.bc[i] = g;
  }
}

// Hll_p and b_p of point p: its edges in ascending k, serially
RGBL_HD void lba_point_sums(const LbaView& V, int p) {
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  for (int k = V.pt_off[p]; k < V.pt_off[p + 1]; ++k) {
    const LbaEdgeLin& L = V.lin[k];
    for (int i = 0; i < 6; ++i) H[i] = H[i] + L.Hll[i];
    for (int i = 0; i < 3; ++i) b[i] = b[i] + L.bp[i];
  }
  for (int i = 0; i < 6; ++i) V.pt_H[6 * (size_t)p + i] = H[i];
  for (int i = 0; i < 3; ++i) V.pt_b[3 * (size_t)p + i] = b[i];
}

// what lane `lane` of column a's 64 adds to its 27 partial sums (Hpp 21, b 6)
RGBL_HD void lba_cam_lane(const LbaView& V, int a, int lane, double acc[27]) {
  for (int i = 0; i < 27; ++i) acc[i] = 0.0;
  for (int j = V.cam_eoff[a] + lane; j < V.cam_eoff[a + 1]; j += kLbaCamLanes) {
    const LbaEdgeLin& L = V.lin[V.cam_edges[j]];
    for (int i = 0; i < 21; ++i) acc[i] = acc[i] + L.Hpp[i];
    for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + L.bc[i];
  }
}

// (Hll_p + lambda I)^-1 as Eigen inverts a 3 x 3 matrix (compute_inverse_size3: cofactors, the determinant along column 0)
RGBL_HD void lba_dinv(const double* H, double lambda, double Di[9]) {
  const double m[3][3] = {{H[0] + lambda, H[1], H[2]}, {H[1], H[3] + lambda, H[4]}, {H[2], H[4], H[5] + lambda}};
  double c[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      c[i][j] = m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    }
  const double det = (c[0][0] * m[0][0] + c[1][0] * m[1][0]) + c[2][0] * m[2][0];
  const double invdet = 1.0 / det;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Di[3 * i + j] = c[j][i] * invdet;
}

// the trial's per-edge products (block_solver.hpp:396-408): BDinv = B Dinv, and B (Dinv b_p).  Edges of fixed cameras have none.
RGBL_HD void lba_trial_edge(const LbaView& V, double lambda, int k) {
  if (V.col[V.e_cam[k]] < 0) return;
  const int p = V.e_pt[k];
  double Di[9], db[3];
  lba_dinv(V.pt_H + 6 * (size_t)p, lambda, Di);
  const double* b = V.pt_b + 3 * (size_t)p;
  for (int i = 0; i < 3; ++i) db[i] = (Di[3 * i] * b[0] + Di[3 * i + 1] * b[1]) + Di[3 * i + 2] * b[2];
  const double* W = V.lin[k].W;
  LbaEdgeTrial& R = V.tr[k];
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 3; ++j) R.BD[3 * i + j] = (W[3 * i] * Di[j] + W[3 * i + 1] * Di[3 + j]) + W[3 * i + 2] * Di[6 + j];
    R.Bdb[i] = (W[3 * i] * db[0] + W[3 * i + 1] * db[1]) + W[3 * i + 2] * db[2];
  }
}

// Work-item t of upper block blk = (i, j).  t < 36: entry (t / 6, t % 6) of S_ij over the block's pairs in ascending point
// order, stored into the solver's lower triangle at (6 j + b, 6 i + a).  t = 36 .. 41, diagonal blocks: row t - 36 of coeff_i
// over column i's edges, and b_schur.
RGBL_HD void lba_schur_lane(const LbaView& V, double lambda, int i, int j, int t) {
  const int blk = lba_block(V.nA, i, j);
  if (t < 36) {
    const int a = t / 6, b = t % 6;
    if (i == j && a > b) return;
    double v = 0.0;
    if (i == j) {
      v = V.cam_H[21 * (size_t)i + LmSystem<6>::diag(a) + (b - a)];
      if (a == b) v = v + lambda;
    }
    for (int q = V.blk_off[blk]; q < V.blk_off[blk + 1]; ++q) {
      const double* BD = V.tr[V.pairs[2 * (size_t)q]].BD + 3 * a;
      const double* W = V.lin[V.pairs[2 * (size_t)q + 1]].W + 3 * b;
      v = v - ((BD[0] * W[0] + BD[1] * W[1]) + BD[2] * W[2]);
    }
    V.S[lm_tri((size_t)(6 * j + b), (size_t)(6 * i + a))] = v;
  } else if (t < 42 && i == j) {
    const int r = t - 36;
    double coeff = 0.0;
    for (int q = V.cam_eoff[i]; q < V.cam_eoff[i + 1]; ++q) coeff = coeff + V.tr[V.cam_edges[q]].Bdb[r];
    V.bs[6 * i + r] = V.cam_b[6 * (size_t)i + r] - coeff;
  }
}

// VertexSE3Expmap::oplusImpl of column a with the solver's x
RGBL_HD void lba_trial_camera(const LbaView& V, int a) {
  const int c = V.col_cam[a];
  V.Tt[c] = po_oplus(V.x_cam + 6 * (size_t)a, V.T[c]);
}

// Point p of a trial: after a successful factorisation its part of x (block_solver.hpp:461-480), else the x it holds; the
// trial estimate (VertexSBAPointXYZ::oplusImpl), and the chi2 of its edges there.
RGBL_HD void lba_trial_point(const LbaView& V, double lambda, bool ok, int p) {
  double* xp = V.x_pt + 3 * (size_t)p;
  if (ok) {
    double Di[9], c[3];
    lba_dinv(V.pt_H + 6 * (size_t)p, lambda, Di);
    for (int i = 0; i < 3; ++i) c[i] = V.pt_b[3 * (size_t)p + i];
    for (int k = V.pt_off[p]; k < V.pt_off[p + 1]; ++k) {
      const int a = V.col[V.e_cam[k]];
      if (a < 0) continue;
      const double* W = V.lin[k].W;
      const double* x = V.x_cam + 6 * (size_t)a;
      for (int j = 0; j < 3; ++j)
        c[j] = c[j] - (((((W[j] * x[0] + W[3 + j] * x[1]) + W[6 + j] * x[2]) + W[9 + j] * x[3]) + W[12 + j] * x[4]) + W[15 + j] * x[5]);
    }
    for (int i = 0; i < 3; ++i) xp[i] = (Di[3 * i] * c[0] + Di[3 * i + 1] * c[1]) + Di[3 * i + 2] * c[2];
  }
  for (int i = 0; i < 3; ++i) V.Xt[3 * (size_t)p + i] = V.X[3 * (size_t)p + i] + xp[i];
  for (int k = V.pt_off[p]; k < V.pt_off[p + 1]; ++k) lba_edge_chi2(V, k, V.Tt, V.Xt);
}

// The whole-system sums, lane by lane.  what 0: the robust chi2 over the edges; 1: computeScale over the unknowns; 2: the
// largest |diagonal| over the unknowns (combine with lba_max).
RGBL_HD double lba_max(double a, double m) { return (a < m) ? m : a; }   // std::max(a, m)
RGBL_HD int lba_unknowns(const LbaView& V) { return V.n + 3 * V.nPa; }
RGBL_HD double lba_sum_lane(const LbaView& V, int what, double lambda, int lane) {
  double acc = 0.0;
  if (what == 0) {
    for (int k = lane; k < V.nE; k += kLmLanes) acc = acc + V.e_rho[k];
    return acc;
  }
  const int nU = lba_unknowns(V);
  for (int u = lane; u < nU; u += kLmLanes) {
    double x, b, h;
    if (u < V.n) {
      x = V.x_cam[u]; b = V.cam_b[u];
      h = V.cam_H[21 * (size_t)(u / 6) + LmSystem<6>::diag(u % 6)];
    } else {
      const int p = V.act_pt[(u - V.n) / 3], r = (u - V.n) % 3;
      x = V.x_pt[3 * (size_t)p + r]; b = V.pt_b[3 * (size_t)p + r];
      h = V.pt_H[6 * (size_t)p + (r == 0 ? 0 : r == 1 ? 3 : 5)];
    }
    if (what == 1) acc = acc + x * (lambda * x + b);
    else acc = lba_max(fabs(h), acc);
  }
  return acc;
}

// :1417-1460 for edge k at the final estimates: bit 0 = erase (chi2 beyond the threshold, or a depth that is not positive),
// bit 1 = the depth is not positive
RGBL_HD void lba_flag_edge(const LbaView& V, int k) {
  const int p = V.e_pt[k], c = V.e_cam[k];
  double P[3];
  po_map(V.T[c], V.X + 3 * (size_t)p, P);
  const bool behind = !(P[2] > 0.0);
  const bool beyond = V.e_chi2[k] > (lba_stereo(V.e_obs + 3 * (size_t)k) ? 7.815 : 5.991);
  V.flags[k] = (uint8_t)(((beyond || behind) ? 1 : 0) | (behind ? 2 : 0));
}

// ---- Levenberg's scalar control -----------------------------------------------------------------------------------------
// terminate() (sparse_optimizer.cpp: _forceStopFlag && *_forceStopFlag).  `after` > 0: the flag reads as set from that poll on.
struct LbaStop {
  const volatile int32_t* flag;
  const volatile uint8_t* byte;   // the same flag as a C++ bool
  int after, polls;
  RGBL_HD bool poll() {
    ++polls;
    if (after > 0 && polls >= after) return true;
    return (flag && *flag != 0) || (byte && *byte != 0);
  }
};
typedef LmCounters LbaCounters;

// Levenberg's scalar control is lm_levenberg_loop of lm_math.h, the text PoseOptimization's and OptimizeSim3's vertex runs
// too; the policy's linearise(first, &chi, &maxdiag), trial(lambda, &ok, &chi, &scale) and accept() are kernel launches with
// one record read back (csrc/lba.hip) or the host's loops, and computeLambdaInit's maximum runs over ALL active vertices.

}  // namespace rgbl
