"""Per-call latency of Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) - two key frames of 2 000 features, host arrays in,
host arrays out - at 30, 150 and 500 correspondences, one candidate per call (rgbl_optimize_sim3) and the 8 candidates of a
DetectCommonRegionsFromBoW pass in one call (rgbl_optimize_sim3_batch).

For each: the wall time of the C call (time.perf_counter around the prepared ctypes call, synchronous; 10 warm-up calls, then
the median, minimum and 90th percentile of --calls calls), its kernel time (the handle's HIP-event profile, a separate set of
calls), and beside it the HOST build of csrc/sim3opt_math.h on one core (rgbl_optimize_sim3_host on the same problems).  That
host figure is THIS PROJECT'S restatement, not g2o: nobody has measured g2o for this function on this machine, and no speed-up
against the reference follows from these numbers.  The function had no device form before, so there is no earlier figure.

    python tools/sim3_opt_bench.py [--n 2000] [--calls 200] [--out profiles/sim3_opt_calls.json]      on the MI355X

One JSON line on stdout; --out writes the result under the key "device".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_rgbl_amd import sim3_cases as sc  # noqa: E402


def stats(t):
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call, calls, warm=10):
    t = []
    for _ in range(calls + warm):
        a = time.perf_counter()
        call()
        t.append((time.perf_counter() - a) * 1e6)
    return stats(t[warm:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)

    def measure(problems, calls):
        call = mt.prepare_OptimizeSim3Batch(problems)
        got, want = call(), mt.OptimizeSim3Batch(problems, host=True)
        for g, w in zip(got, want):   # the same bits, or the figures below compare different things
            assert g["result"] == w["result"] and np.array_equal(g["cleared"], w["cleared"]) and g["q"].tobytes() == w["q"].tobytes()
        wall = timed(call.c_call, calls)
        mt.profile(True)
        for _ in range(20):
            call.c_call()
        ms, cnt = mt.profile_read()["k_sim3_opt"]
        mt.profile(False)
        host = timed(call.c_call_host, max(5, calls // 4), warm=2)
        return dict(problems=len(problems), correspondences=[g["n_correspondences"] for g in got][:4], inliers=[g["result"] for g in got][:4],
                    dropped=[g["n_bad"] for g in got][:4], levenberg_iterations=[int(g["iterations"].sum()) for g in got][:4],
                    call=wall, kernel_us=round(ms / max(cnt, 1) * 1e3, 1), host_build_one_core=host)

    result = dict(what="Optimizer::OptimizeSim3, two key frames of %d features, host arrays in and out, synchronous; median of %d calls "
                       "after 10 warm-up calls.  host_build_one_core is this project's restatement (csrc/sim3opt_math.h compiled for "
                       "the host), NOT g2o" % (args.n, args.calls), n=args.n)
    for m in (30, 150, 500):
        result[str(m)] = dict(single=measure([sc.make_sim3_opt_case(args.n, m, seed=3)], args.calls),
                              batch_of_8=measure([sc.make_sim3_opt_case(args.n, m, seed=100 + b) for b in range(8)], args.calls))
    mt.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": result}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
