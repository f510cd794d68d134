// rgbl::so_exp (csrc/sim3opt_math.h) against the live libm's exp.  tests/test_sim3_opt_math.py builds and runs this twice: plain,
// and with -fsanitize=address,undefined -fno-sanitize-recover=undefined - the stand-alone sanitizer run of the header's host build.
//   small   2^22 arguments evenly spaced over [0, 1] and their negatives: what sigma of an update can be
//   wide    2^22 arguments evenly spaced over [-745.2, 709.8], the whole range with a finite, non-zero result
// Prints, per range, the largest difference in units of the libm result's last place and how many results differ at all; then
// the special values; then one small problem through so_optimize on the host lanes (every function of the header is run).
// Built with -ffp-contract=off -fno-builtin.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../orb_slam3_rgbl_amd/csrc/sim3opt_math.h"

static double ulps(double got, double want) {
  if (got == want) return 0.0;
  const double ulp = nextafter(fabs(want), INFINITY) - fabs(want);
  return fabs(got - want) / ulp;
}

struct Worst { double u = 0.0, at = 0.0; uint64_t differ = 0; };
static void take(Worst& w, double x) {
  const double u = ulps(rgbl::so_exp(x), exp(x));
  if (u > 0.0) ++w.differ;
  if (u > w.u) { w.u = u; w.at = x; }
}

int main() {
  const int N = 1 << 22;
  Worst small, wide;
  for (int i = 0; i <= N; ++i) {
    take(small, 1.0 * i / N);
    take(small, -1.0 * i / N);
  }
  for (int i = 0; i <= N; ++i) take(wide, -745.2 + (709.8 + 745.2) * i / N);
  printf("small exp max_ulp %.3f at %a differ %llu\n", small.u, small.at, (unsigned long long)small.differ);
  printf("wide exp max_ulp %.3f at %a differ %llu\n", wide.u, wide.at, (unsigned long long)wide.differ);
  const bool special = rgbl::so_exp(0.0) == 1.0 && rgbl::so_exp(-0.0) == 1.0 && rgbl::so_exp(INFINITY) == INFINITY &&
                       rgbl::so_exp(-INFINITY) == 0.0 && rgbl::so_exp(NAN) != rgbl::so_exp(NAN) && rgbl::so_exp(710.0) == INFINITY &&
                       rgbl::so_exp(-746.0) == 0.0 && rgbl::so_exp(1e-300) == 1.0 && rgbl::so_exp(-740.0) > 0.0 &&
                       rgbl::so_exp(-740.0) == exp(-740.0);
  printf("special values %d\n", special ? 1 : 0);

  // twenty points in front of two cameras one metre apart, the entry estimate off by a few centimetres
  using namespace rgbl;
  const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
  const SoCam C = {700.0, 700.0, 600.0, 180.0};
  std::vector<SoEdge> edges;
  for (int i = 0; i < 20; ++i) {
    const float X1[3] = {(float)(i % 5) - 2.0f, (float)(i / 5) - 1.5f, 8.0f + (float)i};
    const float X2[3] = {X1[0] - 1.0f, X1[1], X1[2]};   // X1 = X2 + (1, 0, 0)
    const float kp1[2] = {(float)(C.fx * X1[0] / X1[2] + C.cx), (float)(C.fy * X1[1] / X1[2] + C.cy)};
    const float kp2[2] = {(float)(C.fx * X2[0] / X2[2] + C.cx) + (i == 7 ? 40.0f : 0.0f), (float)(C.fy * X2[1] / X2[2] + C.cy)};
    SoEdge e;
    if (so_make_edge(I, zero, I, zero, X1, X2, kp1, 1.0f, true, kp2, 1.0f, e)) edges.push_back(e);
  }
  std::vector<SoHostLanes> lanes(1, SoHostLanes(edges.data(), (int)edges.size()));
  const SoSim3 entry = {{0.0, 0.01, 0.0, 1.0}, {1.03, -0.02, 0.01}, 1.02};
  SoSim3 out;
  SoDiag diag;
  memset(&diag, 0, sizeof(diag));
  const int n_in = so_optimize(lanes[0], C, C, entry, (int)edges.size(), 10.0f, false, out, diag);
  printf("optimised: nIn %d of %d, dropped %d, iterations %d + %d, t = %.6f %.6f %.6f, s = %.6f\n", n_in, (int)edges.size(), diag.n_bad,
         diag.iterations[0], diag.iterations[1], out.t[0], out.t[1], out.t[2], out.s);
  const bool solved = n_in == 19 && diag.n_bad == 1 && fabs(out.t[0] - 1.0) < 1e-3 && fabs(out.s - 1.0) < 1e-3;
  return special && solved ? 0 : 1;
}
