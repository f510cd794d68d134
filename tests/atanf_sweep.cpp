// rgbl::np_atanf / np_atan2f / np_cos_parallax_stereo (csrc/newpoint_math.h) against the live libm, bit for bit
// (tests/test_new_points_math.py builds and runs this):
//   atan    every float of [2^-14, 2^14], and every 2^10-th float of both signs outside (zeros, subnormals, inf, NaNs)
//   atan2   atan2f(h, d) for every float d of [0.25, 512] and h = mb / 2 of five baselines 0.1 - 1.1 m; every 2^10-th float
//           d of both signs for one of them, and the special pairs of e_atan2f.c
//   cos     cosf(2 * atan2f(h, d)) on the atan2 mode's arguments at a stride of 7
// Prints "checked N mismatches M" and the first mismatching inputs.  NaN results are compared as NaN, not by payload.
// Built with -ffp-contract=off -fno-builtin: the restatement is not contracted and atanf really is the library's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../orb_slam3_rgbl_amd/csrc/newpoint_math.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static bool same(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }

struct Tally {
  std::atomic<uint64_t> checked{0}, mismatches{0};
  std::mutex mu;
  std::vector<std::pair<uint32_t, uint32_t>> first;
  void miss(uint32_t a, uint32_t b) {
    ++mismatches;
    std::lock_guard<std::mutex> lock(mu);
    if (first.size() < 32) first.push_back({a, b});
  }
};

// body(j) for j in [0, total) over 16 threads
static void sweep(uint64_t total, const std::function<void(uint64_t)>& body) {
  const int nthreads = 16;
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&, t]() {
      for (uint64_t j = total * t / nthreads, e = total * (t + 1) / nthreads; j < e; ++j) body(j);
    });
  for (auto& th : pool) th.join();
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "atan";
  Tally T;
  const float halves[5] = {0.05f, 0.15f, 0.2686f, 0.4f, 0.55f};
  if (strcmp(mode, "atan") == 0) {
    const uint32_t lo = bits(0x1p-14f), hi = bits(0x1p14f);
    sweep((uint64_t)hi - lo + 1, [&](uint64_t j) {
      const uint32_t u = (uint32_t)(lo + j);
      if (!same(rgbl::np_atanf(from_bits(u)), atanf(from_bits(u)))) T.miss(u, 0);
    });
    T.checked += (uint64_t)hi - lo + 1;
    sweep(1u << 22, [&](uint64_t j) {
      const uint32_t u = (uint32_t)(j << 10);
      if (!same(rgbl::np_atanf(from_bits(u)), atanf(from_bits(u)))) T.miss(u, 0);
    });
    T.checked += 1u << 22;
  } else {
    const bool with_cos = strcmp(mode, "cos") == 0;
    auto one = [&](float h, float d) {
      const float got = rgbl::np_atan2f(h, d), want = atan2f(h, d);
      if (!same(got, want)) { T.miss(bits(h), bits(d)); return; }
      if (with_cos && !same(rgbl::np_cos_parallax_stereo(2.0f * h, d), cosf(2.0f * want))) T.miss(bits(h), bits(d));
    };
    const uint32_t lo = bits(0.25f), hi = bits(512.f), step = with_cos ? 7 : 1;
    const uint64_t n = ((uint64_t)hi - lo) / step + 1;
    for (float h : halves) {
      sweep(n, [&](uint64_t j) { one(h, from_bits((uint32_t)(lo + j * step))); });
      T.checked += n;
    }
    sweep(1u << 22, [&](uint64_t j) { one(halves[2], from_bits((uint32_t)(j << 10))); });
    T.checked += 1u << 22;
    const float sp[] = {0.f, -0.f, 1.f, -1.f, INFINITY, -INFINITY, NAN, 1e-30f, -1e-30f, 1e30f, -1e30f, 0.2686f, 3.f};
    for (float y : sp)
      for (float x : sp) { one(y, x); ++T.checked; }
  }
  printf("checked %llu mismatches %llu\n", (unsigned long long)T.checked.load(), (unsigned long long)T.mismatches.load());
  for (auto& p : T.first) printf("  0x%08x 0x%08x\n", p.first, p.second);
  return T.mismatches.load() ? 1 : 0;
}
