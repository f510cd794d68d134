// rgbl::logf_glibc against the live libm's logf, bit for bit (tests/test_logf_glibc.py builds and runs this):
//   dense   every float of [2^-12, 2^12]
//   sparse  every 2^10-th positive float outside that range (subnormals, huge values, inf, the NaNs behind it)
// Prints "checked N mismatches M" and the first mismatching inputs.  NaN results are compared as NaN, not by payload.
// Built with -ffp-contract=off -fno-builtin: the restatement is not contracted and logf really is the library's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "../orb_slam3_rgbl_amd/csrc/logf_glibc.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static bool same(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }

int main(int argc, char** argv) {
  const bool dense = argc > 1 && strcmp(argv[1], "dense") == 0;
  const int nthreads = 16;
  const uint32_t lo = bits(0x1p-12f), hi = bits(0x1p12f);
  std::vector<uint32_t> inputs;  // sparse mode only
  if (!dense)
    for (uint64_t u = 0; u <= 0x7fffffffull; u += 1024)
      if (u < lo || u > hi) inputs.push_back((uint32_t)u);
  const uint64_t total = dense ? (uint64_t)hi - lo + 1 : inputs.size();
  std::atomic<uint64_t> mismatches{0};
  std::mutex mu;
  std::vector<uint32_t> first;
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; ++t)
    pool.emplace_back([&, t]() {
      const uint64_t b = total * t / nthreads, e = total * (t + 1) / nthreads;
      for (uint64_t j = b; j < e; ++j) {
        const uint32_t u = dense ? (uint32_t)(lo + j) : inputs[j];
        const float x = from_bits(u);
        if (same(rgbl::logf_glibc(x), logf(x))) continue;
        ++mismatches;
        std::lock_guard<std::mutex> lock(mu);
        if (first.size() < 32) first.push_back(u);
      }
    });
  for (auto& th : pool) th.join();
  printf("checked %llu mismatches %llu\n", (unsigned long long)total, (unsigned long long)mismatches.load());
  for (uint32_t u : first) {
    const float x = from_bits(u);
    printf("  x = 0x%08x (%a): restatement 0x%08x, libm 0x%08x\n", u, x, bits(rgbl::logf_glibc(x)), bits(logf(x)));
  }
  return mismatches.load() ? 1 : 0;
}
