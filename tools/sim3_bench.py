"""Per-call latency of Sim3Solver (src/Sim3Solver.cc) on the device - every hypothesis of a call at once - at loop-closing size:
n = 150 correspondences, 300 hypotheses, min_inliers = n (the scan runs through: the whole call's work, no early stop):

    single   rgbl_sim3_ransac, B = 1
    batch    rgbl_sim3_ransac_batch, B = 8 candidates of one DetectCommonRegionsFromBoW pass (other sizes with --batches)

For each: the wall time of the C call (time.perf_counter around the prepared ctypes call: host arrays in, host arrays out, the
call ends in a stream synchronise), warmed up, median / min / p10 / p90 over --calls repetitions; the two kernels' times from the
handle's HIP-event profile (a separate set of calls; an event pair around a kernel of a few microseconds measures mostly itself,
so DESIGN.md's kernel columns come from a kernel trace instead: one setting per run, nothing else traced,

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sim3_bench.py --batches 8 --sizes ""

); and beside it the HOST build of csrc/sim3_math.h on one core (rgbl_sim3_ransac_host on the same problems).
That host figure is THIS PROJECT'S restatement, not Eigen's EigenSolver and not the reference: nobody has measured the
reference's Sim3Solver on this machine, and no speed-up against it follows from these numbers.

    python tools/sim3_bench.py [--n 150] [--hyp 300] [--calls 300] [--out profiles/sim3_calls.json]      on the MI355X

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
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p10_us=round(float(np.percentile(t, 10)), 1),
                p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call, calls, warm=20):
    t = []
    for _ in range(calls + warm):
        a = time.perf_counter()
        call()
        t.append((time.perf_counter() - a) * 1e6)
    return stats(t[warm:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150)
    ap.add_argument("--hyp", type=int, default=300)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--sizes", default="20,50,150,500", help="n of the single-problem sweep that locates the host / device crossover")
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)

    def measure(n, B, calls):
        prs = [sc.problem(sc.make_sim3_case(n, args.hyp, seed=50 + b, min_inliers=n)) for b in range(B)]
        call = mt.prepare_Sim3RansacBatch(prs, diag=False)
        got, want = call(), mt.prepare_Sim3RansacBatch(prs, host=True, diag=False)()
        for g, w in zip(got, want):   # the same bits, or the figures below compare different things
            assert g["selected"] == w["selected"] >= 0 and np.array_equal(g["inlier"], w["inlier"]) and g["T12"].tobytes() == w["T12"].tobytes()
        wall = timed(call.c_call, calls)
        host = timed(call.c_call_host, max(10, calls // 10), warm=3)
        mt.profile(True)
        for _ in range(20):
            call.c_call()
        prof = mt.profile_read()
        mt.profile(False)
        kern = {k: round(prof[k][0] / max(prof[k][1], 1) * 1e3, 1) for k in ("k_sim3_hypotheses", "k_sim3_select")}
        return dict(n=n, hypotheses=args.hyp, problems=B, inliers=[g["n_inliers"] for g in got][:4], call=wall, kernel_us=kern,
                    host_build_one_core=host)

    result = dict(what="Sim3Solver, every hypothesis of a call at once; host arrays in and out, synchronous; %d calls after 20 warm-up "
                       "calls.  host_build_one_core is this project's restatement (csrc/sim3_math.h compiled for the host), NOT the "
                       "reference's Sim3Solver with Eigen" % args.calls)
    result["batch"] = {str(B): measure(args.n, B, args.calls) for B in [int(v) for v in args.batches.split(",") if v]}
    result["single_by_n"] = {str(n): measure(n, 1, max(50, args.calls // 3)) for n in [int(v) for v in args.sizes.split(",") if v]}
    mt.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": result}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
