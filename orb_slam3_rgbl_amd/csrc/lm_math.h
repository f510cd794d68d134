// lm_math.h — the part of g2o that Optimizer::PoseOptimization (csrc/poseopt_math.h, 6 unknowns) and Optimizer::OptimizeSim3
// (csrc/sim3opt_math.h, 7 unknowns) both run, in ONE place for host and device: the layout of a reduced system, the dense
// solve, OptimizationAlgorithmLevenberg::solve and the lanes' summation order, restated from
//   Thirdparty/g2o/g2o/core/{optimization_algorithm_levenberg,sparse_optimizer}.cpp, solvers/linear_solver_dense.h
// All arithmetic is fp64, no contraction.  OptimizeSim3 calls lm_levenberg; po_optimize carries that loop written out (it says why).
// lm_solve_n is lm_solve for a run-time n; csrc/lba_math.h (LocalBundleAdjustment) solves its reduced camera system with it and
// runs lm_levenberg_loop with its own policy: kernel launches (csrc/lba.hip) or host loops, and the caller's stop flag.
// lm_solve_panel is lm_solve_n in panels of columns with the backward substitution mirrored: the reduced system of the global
// bundle adjustment (csrc/gba.hip), which is too large for one workgroup and for lm_solve_n's backward order.
//
// What is NOT pinned: Eigen's LDLT with its pivoting, replaced by lm_solve (LDL^T without pivoting).  Deviations that follow
// from the solver and are kept on purpose, for both optimisers:
//   - a pivot that is not finite and > 0 counts as a failed factorisation (LDLT::isPositive() also accepts zero pivots);
//   - after a failed factorisation g2o's x keeps whatever it held (uninitialised memory before the first success); here x is
//     the caller's, starts as zeros on entry and persists across failed factorisations, trials, iterations and rounds.
// Quirks of g2o's Levenberg that ARE kept, for both:
//   - a failed factorisation gives tempChi = DBL_MAX, which passes g2o_isfinite: with an infinite currentChi rho is +inf and
//     the step - the x of the last successful solve, or zeros - is ACCEPTED;
//   - the edges keep the chi2 of the last TRIED step, even a rejected one (pop() restores the vertex, not the edges' errors).
//
// Summation order (host, emulator and GPU agree bit for bit).  Edge k, in ascending feature index, belongs to lane k mod 256;
// a lane adds its edges in ascending k; the 256 partial sums are combined by the fixed tree v[i] = v[i] + v[i + s] for
// s = 128, 64, ..., 1.  This holds for every sum of a system and for every single sum.  LmHostLanes below is the host's
// execution of it, lm_tree_reduce of csrc/optimize.hip the workgroup's.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef RGBL_HD
#if defined(__HIPCC__)
#define RGBL_HD __host__ __device__ inline
#else
#define RGBL_HD inline
#endif
#endif
// the Levenberg loop and its dense policy dissolve into the kernel that runs them
#ifndef RGBL_HD_FLAT
#if defined(__HIPCC__)
#define RGBL_HD_FLAT __host__ __device__ __forceinline__
#else
#define RGBL_HD_FLAT inline
#endif
#endif

namespace rgbl {

constexpr int kLmLanes = 256;   // work-items of one problem
constexpr int kLmTrials = 10;   // _maxTrialsAfterFailure (optimization_algorithm_levenberg.cpp:46)
constexpr int kLmPanel = 32;    // columns of a panel of lm_solve_panel on the device (csrc/gba.hip; DESIGN.md 9 has the measurement)

// A reduced system of N unknowns: H's upper triangle row by row, then b, then the robust chi2.
template <int N> struct LmSystem {
  static constexpr int kB = N * (N + 1) / 2, kChi = kB + N, kSums = kChi + 1;
  static constexpr int diag(int j) { return j * N - j * (j - 1) / 2; }   // H[j][j]: rows of N, N - 1, ... entries lie before it
};

// (H + lambda I) x = b by LDL^T without pivoting; Hu = the upper triangle row by row.  False, x untouched, when a pivot is not
// finite and > 0 (linear_solver_dense.h:107-109: LDLT::isPositive() false).
template <int N> RGBL_HD bool lm_solve(const double* Hu, double lambda, const double* b, double* x) {
  double L[N][N], D[N], y[N];
  int k = 0;
  #pragma unroll
  for (int j = 0; j < N; ++j)
    #pragma unroll
    for (int c = j; c < N; ++c, ++k) L[c][j] = Hu[k] + (c == j ? lambda : 0.0);   // lower triangle of the symmetric matrix
  #pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = L[j][j];
    #pragma unroll
    for (int p = 0; p < j; ++p) d = d - L[j][p] * L[j][p] * D[p];
    if (!(d > 0.0 && d <= DBL_MAX)) return false;
    D[j] = d;
    #pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = L[i][j];
      #pragma unroll
      for (int p = 0; p < j; ++p) v = v - L[i][p] * L[j][p] * D[p];
      L[i][j] = v / d;
    }
  }
  #pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = b[i];
    #pragma unroll
    for (int p = 0; p < i; ++p) v = v - L[i][p] * y[p];
    y[i] = v;
  }
  #pragma unroll
  for (int i = 0; i < N; ++i) y[i] = y[i] / D[i];
  #pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = y[i];
    #pragma unroll
    for (int p = i + 1; p < N; ++p) v = v - L[p][i] * x[p];
    x[i] = v;
  }
  return true;
}

// lm_solve for a run-time n (csrc/lba_math.h: the reduced camera system of LocalBundleAdjustment).  A holds the LOWER triangle
// row by row - element (i, j), j <= i, at i (i + 1) / 2 + j -, the diagonal already with its lambda, and is overwritten with L
// (the diagonal entries with the pivots).  D and y are scratch of n doubles.  Every element is formed exactly as lm_solve<N>
// forms it: a - sum_p (L_ip * L_jp) * D_p with p ascending, subtracted one at a time; forward, diagonal and backward
// substitution in lm_solve's order.  A schedule that computes whole elements in parallel (k_lba_factor) gives the same bits.
// False, x untouched, when a pivot is not finite and > 0.
RGBL_HD size_t lm_tri(size_t i, size_t j) { return i * (i + 1) / 2 + j; }
inline bool lm_solve_n(int n, double* A, const double* b, double* x, double* D, double* y) {
  for (int j = 0; j < n; ++j) {
    const double* Lj = A + lm_tri((size_t)j, 0);
    double d = Lj[j];
    for (int p = 0; p < j; ++p) d = d - Lj[p] * Lj[p] * D[p];
    if (!(d > 0.0 && d <= DBL_MAX)) return false;
    D[j] = d;
    for (int i = j + 1; i < n; ++i) {
      double* Li = A + lm_tri((size_t)i, 0);
      double v = Li[j];
      for (int p = 0; p < j; ++p) v = v - Li[p] * Lj[p] * D[p];
      Li[j] = v / d;
    }
  }
  for (int i = 0; i < n; ++i) {
    const double* Li = A + lm_tri((size_t)i, 0);
    double v = b[i];
    for (int p = 0; p < i; ++p) v = v - Li[p] * y[p];
    y[i] = v;
  }
  for (int i = 0; i < n; ++i) y[i] = y[i] / D[i];
  for (int i = n - 1; i >= 0; --i) {
    double v = y[i];
    for (int p = i + 1; p < n; ++p) v = v - A[lm_tri((size_t)p, (size_t)i)] * x[p];
    x[i] = v;
  }
  return true;
}

// lm_solve_n in panels of w columns, with the backward substitution in the MIRRORED order: the solve of the global bundle
// adjustment (csrc/gba.hip), whose reduced system reaches n = 6 144.  Per element:
//   factorisation           unchanged: a - sum_p (L_ip * L_jp) * D_p, p ascending, subtracted one at a time; the division by the
//                           pivot and the pivot test d > 0 && d <= DBL_MAX as in lm_solve_n
//   forward substitution    unchanged: y_i = b_i - sum_p L_ip y_p, p ascending; then y_i / D_i
//   backward substitution   x_i = y_i - sum_p L_pi x_p with p DESCENDING from n - 1 to i + 1, the mirror of the forward sweep
// The backward order is the only difference to lm_solve_n, and it is there for the schedule: with p ascending the first term of
// x_i needs x_{i+1} final and the last term of x_{i+1} is p = n - 1, n (n - 1) / 2 dependent subtractions whatever the schedule
// (1.9e7 at n = 6 144; k_lba_factor's work-item 0 runs them alone).  Descending, x_i's terms arrive in the order the x_p become
// final, and a finished block of w values is applied to every row above it in parallel.  The factorisation and the forward
// sweep have no such chain: every element is a sum over values that are already final, so the panel schedule below - (a) the
// panel's columns through every p before the panel, (b) its w x w diagonal block, (c) the rows below, then the substitutions
// block by block - forms lm_solve_n's L, D and y bit for bit, for every w >= 1.  The kernels of csrc/gba.hip run these loops
// with an element, or a row, per work-item; they run (a) in slices - behind every finished panel all later columns continue
// their sums through that panel's w columns and are stored back, which is the same p ascending per element and spreads over
// the whole trailing matrix instead of one panel's columns.  A as in lm_solve_n, but the diagonal entries end as the pivots.
// False, x untouched, when a pivot is not finite and > 0.
inline bool lm_solve_panel(int n, int w, double* A, const double* b, double* x, double* D, double* y) {
  for (int j0 = 0; j0 < n; j0 += w) {
    const int j1 = j0 + w < n ? j0 + w : n;
    for (int i = j0; i < n; ++i) {                       // (a)
      double* Li = A + lm_tri((size_t)i, 0);
      for (int j = j0; j < j1 && j <= i; ++j) {
        const double* Lj = A + lm_tri((size_t)j, 0);
        double v = Li[j];
        for (int p = 0; p < j0; ++p) v = v - Li[p] * Lj[p] * D[p];
        Li[j] = v;
      }
    }
    for (int j = j0; j < j1; ++j) {                      // (b)
      double* Lj = A + lm_tri((size_t)j, 0);
      for (int i = j; i < j1; ++i) {
        double* Li = A + lm_tri((size_t)i, 0);
        double v = Li[j];
        for (int p = j0; p < j; ++p) v = v - Li[p] * Lj[p] * D[p];
        Li[j] = v;
      }
      const double d = Lj[j];
      if (!(d > 0.0 && d <= DBL_MAX)) return false;
      D[j] = d;
      for (int i = j + 1; i < j1; ++i) A[lm_tri((size_t)i, (size_t)j)] = A[lm_tri((size_t)i, (size_t)j)] / d;
    }
    for (int i = j1; i < n; ++i) {                       // (c)
      double* Li = A + lm_tri((size_t)i, 0);
      for (int j = j0; j < j1; ++j) {
        const double* Lj = A + lm_tri((size_t)j, 0);
        double v = Li[j];
        for (int p = j0; p < j; ++p) v = v - Li[p] * Lj[p] * D[p];
        Li[j] = v / D[j];
      }
    }
  }
  for (int i = 0; i < n; ++i) y[i] = b[i];
  for (int j0 = 0; j0 < n; j0 += w) {
    const int j1 = j0 + w < n ? j0 + w : n;
    for (int i = j0; i < n; ++i) {                       // the block's triangle (i < j1), then the finished block on the rows below
      const double* Li = A + lm_tri((size_t)i, 0);
      double v = y[i];
      for (int p = j0; p < j1 && p < i; ++p) v = v - Li[p] * y[p];
      y[i] = v;
    }
  }
  for (int i = 0; i < n; ++i) y[i] = y[i] / D[i];
  for (int i = 0; i < n; ++i) x[i] = y[i];
  for (int j0 = n > 0 ? (n - 1) / w * w : 0; j0 >= 0 && n > 0; j0 -= w) {
    const int j1 = j0 + w < n ? j0 + w : n;
    for (int i = j1 - 1; i >= 0; --i) {                  // the block's triangle (i >= j0), then the finished block on the rows above
      double v = x[i];
      for (int p = j1 - 1; p >= j0 && p > i; --p) v = v - A[lm_tri((size_t)p, (size_t)i)] * x[p];
      x[i] = v;
    }
  }
  return true;
}

// ---- Levenberg's scalar control: ONE text for 6, 7 and a run-time number of unknowns -------------------------------------------
// SparseOptimizer::optimize(max_it) (sparse_optimizer.cpp:354-414) with OptimizationAlgorithmLevenberg::solve
// (optimization_algorithm_levenberg.cpp:61-169).  The solve and the passes over the edges are a policy P:
//   P.linearise(first, &chi, &maxdiag)    computeActiveErrors, activeRobustChi2 and buildSystem at the current estimate; for the
//                                         first iteration also computeLambdaInit's largest |diagonal| (:171-185)
//   P.trial(lambda, &ok, &chi, &scale)    setLambda, solve (ok: the factorisation held), update, computeActiveErrors,
//                                         activeRobustChi2 there, and computeScale's sum (:187-194)
//   P.accept()                            discardTop: the trial estimate becomes the current one
// Each returns false to end the loop at once (a device error of a host-driven policy); the function then returns false.
// `stop` is terminate(): polled at the start of every iteration (sparse_optimizer.cpp:376, after i < iterations) and after a
// trial (:149, only when rho < 0 and trials are left).  LmNoStop never stops.  user_lambda_init > 0 replaces computeLambdaInit.
// Every loop is bounded: max_it x kLmTrials trials.
struct LmNoStop { RGBL_HD_FLAT bool poll() { return false; } };
struct LmCounters { int32_t iterations, trials, rejected, failed; double first_chi2, last_chi2, last_lambda; };
template <class Passes, class Stop>
RGBL_HD_FLAT bool lm_levenberg_loop(Passes& P, int max_it, double user_lambda_init, Stop& stop, LmCounters& D) {
  double lambda = 0.0, ni = 2.0, currentChi = 0.0;
  int lmBad = 0;
  D.iterations = D.trials = D.rejected = D.failed = 0;
  D.first_chi2 = D.last_chi2 = D.last_lambda = 0.0;
  for (int it = 0; it < max_it; ++it) {
    if (stop.poll()) break;
    double maxDiagonal = 0.0;
    if (!P.linearise(it == 0, &currentChi, &maxDiagonal)) return false;
    const double iniChi = currentChi;
    double tempChi = currentChi;
    if (it == 0) {                  // computeLambdaInit: _tau = 1e-5
      lambda = user_lambda_init > 0.0 ? user_lambda_init : 1e-5 * maxDiagonal;
      ni = 2.0;
      lmBad = 0;
      D.first_chi2 = currentChi;
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      bool ok = false;
      double scale = 0.0;
      if (!P.trial(lambda, &ok, &tempChi, &scale)) return false;
      ++D.trials;
      if (!ok) { tempChi = DBL_MAX; ++D.failed; }
      rho = currentChi - tempChi;
      scale += 1e-3;
      rho /= scale;
      if (rho > 0.0 && tempChi >= -DBL_MAX && tempChi <= DBL_MAX) {   // g2o_isfinite
        const double c = 2.0 * rho - 1.0;
        double alpha = 1.0 - c * c * c;
        alpha = (2.0 / 3.0 < alpha) ? 2.0 / 3.0 : alpha;                      // std::min(alpha, _goodStepUpperScale)
        const double scaleFactor = (1.0 / 3.0 < alpha) ? alpha : 1.0 / 3.0;   // std::max(_goodStepLowerScale, alpha)
        lambda *= scaleFactor;
        ni = 2.0;
        currentChi = tempChi;
        if (!P.accept()) return false;   // discardTop
      } else {
        lambda *= ni;
        ni *= 2.0;                  // pop: the estimate stays; the edges keep the errors of the rejected step
        ++D.rejected;
      }
      ++qmax;
    } while (rho < 0.0 && qmax < kLmTrials && !stop.poll());
    ++D.iterations;
    D.last_chi2 = currentChi;
    D.last_lambda = lambda;
    if (qmax == kLmTrials || rho == 0.0) break;   // Terminate
    if ((iniChi - currentChi) * 1e3 < iniChi) ++lmBad; else lmBad = 0;   // :157-166
    if (lmBad >= 3) break;
  }
  return true;
}

// The policy of ONE vertex of N unknowns with the dense solve lm_solve<N>.
//   G, the lanes, owns the problem's edges and the partial sums (LmSystem<N>::kSums per lane):
//     G.zero()             every lane's partial sums = 0
//     G.each(f)            f(Edge&, double* acc) for the caller's edges in ascending k (host: every lane in turn)
//     G.reduce_system(buf) the fixed tree over all sums; returns where they stay readable until the next reduce_system():
//                          the caller's buf (kSums doubles) or storage of G's own (k_sim3_opt: LDS)
//     G.reduce_one()       the fixed tree over sum 0
//   M, the optimiser's model, owns the estimate:
//     M.linearise(G)       G.zero() and one pass that adds every active edge's H, b and robust chi2 at the current estimate
//     M.trial(G, x)        forms the trial estimate from x (and may write x: OptimizeSim3's quirk 8); G.zero() and one pass that adds every active edge's robust chi2
//                          there to sum 0
//     M.accept()           the trial estimate becomes the current one
template <int N, class Lanes, class Model> struct LmDensePasses {
  typedef LmSystem<N> Sys;
  Lanes& G;
  Model& M;
  double* x;
  const double* S;
  double sums[Sys::kSums];
  // S must not start as `sums`: with its own array's address in a member the object stays in memory, and k_sim3_opt, whose
  // lanes return LDS from reduce_system, goes from 364 to 1 696 bytes of scratch per lane and loses its 256 AGPRs
  RGBL_HD_FLAT LmDensePasses(Lanes& lanes, Model& model, double* xx) : G(lanes), M(model), x(xx), S(nullptr) {}
  RGBL_HD_FLAT bool linearise(bool first, double* chi, double* maxdiag) {
    M.linearise(G);
    S = G.reduce_system(sums);
    *chi = S[Sys::kChi];
    if (first) {
      double maxDiagonal = 0.0;
      for (int j = 0; j < N; ++j) { const double a = fabs(S[Sys::diag(j)]); maxDiagonal = a > maxDiagonal ? a : maxDiagonal; }   // std::max(fabs, max)
      *maxdiag = maxDiagonal;
    }
    return true;
  }
  RGBL_HD_FLAT bool trial(double lambda, bool* ok, double* chi, double* scale_sum) {
    *ok = lm_solve<N>(S, lambda, S + Sys::kB, x);
    M.trial(G, x);
    *chi = G.reduce_one();
    double scale = 0.0;
    for (int j = 0; j < N; ++j) scale += x[j] * (lambda * x[j] + S[Sys::kB + j]);
    *scale_sum = scale;
    return true;
  }
  RGBL_HD_FLAT bool accept() { M.accept(); return true; }
};

// lm_levenberg_loop on one vertex of N unknowns.  On the device every work-item runs this function; the scalar state
// (lambda, x, ...) is computed redundantly and identically by all of them, so the only synchronisation is inside G.
// *iterations = the solve() calls, *chi = the Levenberg currentChi on return (0 for max_it < 1).
template <int N, class Lanes, class Model>
RGBL_HD_FLAT void lm_levenberg(Lanes& G, Model& M, int max_it, double* x, int* iterations, double* chi) {
  LmDensePasses<N, Lanes, Model> P(G, M, x);
  LmNoStop never;
  LmCounters D;
  lm_levenberg_loop(P, max_it, 0.0, never, D);
  *iterations = D.iterations;
  *chi = D.last_chi2;
}

// The host's execution of the lanes: the partial sums of all 256 lanes side by side, the tree written out.
template <class Edge, int Sums> struct LmHostLanes {
  Edge* e;
  int m;
  double part[kLmLanes][Sums];
  LmHostLanes(Edge* edges, int count) : e(edges), m(count) {}
  void zero() {
    for (int l = 0; l < kLmLanes; ++l)
      for (int c = 0; c < Sums; ++c) part[l][c] = 0.0;
  }
  template <class F> void each(F f) {
    for (int l = 0; l < kLmLanes; ++l)
      for (int k = l; k < m; k += kLmLanes) f(e[k], part[l]);
  }
  void tree(int count) {
    for (int s = kLmLanes / 2; s >= 1; s >>= 1)
      for (int i = 0; i < s; ++i)
        for (int c = 0; c < count; ++c) part[i][c] = part[i][c] + part[i + s][c];
  }
  const double* reduce_system(double* S) {
    tree(Sums);
    for (int c = 0; c < Sums; ++c) S[c] = part[0][c];
    return S;
  }
  double reduce_one() {
    tree(1);
    return part[0][0];
  }
};

}  // namespace rgbl
