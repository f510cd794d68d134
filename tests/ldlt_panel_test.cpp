// lm_solve_panel (orb_slam3_rgbl_amd/csrc/lm_math.h) against lm_solve_n, on the host, stand-alone:
//   - on random symmetric positive definite matrices its L, D and y are lm_solve_n's byte for byte;
//   - its x is the backward sum with p DESCENDING, written out naively here from lm_solve_n's L and y;
//   - a pivot that is not positive at column 0, w - 1, w and n - 1 returns false with x untouched (and lm_solve_n refuses too).
// n runs over {1, 5, w - 1, w, w + 1, 2 w, 2 w + 1, 3 w + 5} for the device's panel width and for 16 and 64.
// Prints LDLT_PANEL_OK and returns 0; tests/test_ldlt_panel.py builds and runs it (also with -fsanitize=address,undefined).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lm_math.h"

using namespace rgbl;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, in (-1, 1)
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// A = B B^T + n I in lm_solve_n's layout: the lower triangle row by row
static std::vector<double> random_spd(int n) {
  std::vector<double> B((size_t)n * n), A(lm_tri((size_t)n, 0));
  for (double& v : B) v = uniform();
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = i == j ? (double)n : 0.0;
      for (int k = 0; k < n; ++k) s += B[(size_t)i * n + k] * B[(size_t)j * n + k];
      A[lm_tri((size_t)i, (size_t)j)] = s;
    }
  return A;
}

static int fail(const char* what, int n, int w, int at) {
  printf("FAILED: %s (n = %d, w = %d, at %d)\n", what, n, w, at);
  return 1;
}

static int check(int n, int w) {
  const std::vector<double> A0 = random_spd(n);
  std::vector<double> b((size_t)n);
  for (double& v : b) v = uniform();
  std::vector<double> A1 = A0, A2 = A0, x1((size_t)n, 7.0), x2((size_t)n, 7.0), D1((size_t)n), D2((size_t)n), y1((size_t)n), y2((size_t)n);
  if (!lm_solve_n(n, A1.data(), b.data(), x1.data(), D1.data(), y1.data())) return fail("lm_solve_n refused an SPD matrix", n, w, 0);
  if (!lm_solve_panel(n, w, A2.data(), b.data(), x2.data(), D2.data(), y2.data())) return fail("lm_solve_panel refused an SPD matrix", n, w, 0);
  for (int i = 0; i < n; ++i) {
    if (memcmp(&D1[(size_t)i], &D2[(size_t)i], 8)) return fail("D differs", n, w, i);
    if (memcmp(&y1[(size_t)i], &y2[(size_t)i], 8)) return fail("y differs", n, w, i);
    if (memcmp(&A2[lm_tri((size_t)i, (size_t)i)], &D2[(size_t)i], 8)) return fail("the diagonal does not hold the pivot", n, w, i);
    for (int j = 0; j < i; ++j)
      if (memcmp(&A1[lm_tri((size_t)i, (size_t)j)], &A2[lm_tri((size_t)i, (size_t)j)], 8)) return fail("L differs", n, w, i);
  }
  std::vector<double> x((size_t)n);
  bool differs_from_ascending = false;
  for (int i = n - 1; i >= 0; --i) {
    double v = y1[(size_t)i];
    for (int p = n - 1; p > i; --p) v = v - A1[lm_tri((size_t)p, (size_t)i)] * x[(size_t)p];
    x[(size_t)i] = v;
    if (memcmp(&x[(size_t)i], &x2[(size_t)i], 8)) return fail("x is not the descending sum", n, w, i);
    differs_from_ascending = differs_from_ascending || memcmp(&x1[(size_t)i], &x2[(size_t)i], 8) != 0;
  }
  if (n >= 2 * w && !differs_from_ascending) return fail("x equals the ascending sum in every bit: the case shows nothing", n, w, 0);
  // a pivot that is not positive
  const int cols[4] = {0, w - 1, w, n - 1};
  for (int c : cols) {
    if (c < 0 || c >= n) continue;
    std::vector<double> Ab = A0, xa((size_t)n, 7.0), xb((size_t)n, 7.0);
    Ab[lm_tri((size_t)c, (size_t)c)] -= D1[(size_t)c] + 1.0;   // the pivot of column c becomes about -1; the earlier ones stay
    std::vector<double> Aa = Ab;
    if (lm_solve_n(n, Aa.data(), b.data(), xa.data(), D1.data(), y1.data())) return fail("lm_solve_n accepted a pivot <= 0", n, w, c);
    if (lm_solve_panel(n, w, Ab.data(), b.data(), xb.data(), D2.data(), y2.data())) return fail("lm_solve_panel accepted a pivot <= 0", n, w, c);
    for (int i = 0; i < n; ++i)
      if (xb[(size_t)i] != 7.0 || xa[(size_t)i] != 7.0) return fail("x was written by a failed factorisation", n, w, c);
  }
  return 0;
}

int main() {
  const int widths[3] = {kLmPanel, 16, 64};
  int bad = 0, cases = 0;
  for (int w : widths) {
    const int sizes[8] = {1, 5, w - 1, w, w + 1, 2 * w, 2 * w + 1, 3 * w + 5};
    for (int n : sizes) { bad += check(n, w); ++cases; }
  }
  if (bad) return 1;
  printf("LDLT_PANEL_OK %d cases, panel width %d\n", cases, kLmPanel);
  return 0;
}
