"""Per-call latency of MLPnPsolver (src/MLPnPsolver.cpp) on the device - every hypothesis of a call at once - at relocalisation
size: N = 100 correspondences per candidate and n_hyp = 35 hypotheses, which is what SetRansacParameters(0.99, 10, 300, 6, 0.5,
5.991) gives (ceil(log 0.01 / log(1 - 0.5^3))), for B = 1, 5 and 15 candidates of one pass of the loop at Tracking.cc:3703, and
one row at n_hyp = 300.  The rows "run_through" use min_inliers = N: no hypothesis can count more than N inliers, so the scan
runs through - the whole call's work; the rows "early_stop" use SetRansacParameters' min_inliers = N / 2 instead (the call then
ends at the first hypothesis with more inliers than that, as a real call does; the device has computed every hypothesis by then,
so the work is the same).

Forms: host arrays in and out, and the resident forms (a DeviceFrame and a MapPointPool: only the indices, samples and state
travel).  For each: the wall time of the C call (time.perf_counter around the prepared ctypes call, which ends in a stream
synchronise), warmed up, median / min / p10 / p90 over --calls repetitions; the two kernels' times from the handle's HIP-event
profile (a separate set of calls); and beside it the HOST build of csrc/mlpnp_math.h on one core (rgbl_mlpnp_ransac_host on the
same problems).  That host figure is THIS PROJECT'S restatement, not the reference: the reference's MLPnPsolver needs Eigen and
has not been built or measured here, and no speed-up against it follows from these numbers.

    python tools/mlpnp_bench.py [--n 100] [--calls 300] [--out profiles/mlpnp_calls.json]      on the MI355X

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
from orb_slam3_rgbl_amd import mlpnp_cases as mc  # noqa: E402


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
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--batches", default="1,5,15")
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)
    keep = []

    def problems(B, n_hyp, min_inliers, resident):
        out = []
        for b in range(B):
            case = mc.make_mlpnp_case(args.n, n_hyp, seed=50 + b, min_inliers=min_inliers)
            pr = mc.problem(case)
            if resident:
                n = len(case["mp_index"])
                fr = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), case["xy"], case["octave"], np.full(n, -1, np.float32))
                keep.append(fr)
                slot = (np.arange(args.n, dtype=np.int32) + b * args.n)
                pool.update(slot, world_pos=case["world_pos"])
                pr = {k: v for k, v in pr.items() if k not in ("xy", "octave", "world_pos")}
                pr.update(device=fr, pool=pool, slot=slot)
            out.append(pr)
        return out

    def measure(B, n_hyp, min_inliers, calls):
        host_prs = problems(B, n_hyp, min_inliers, False)
        call = mt.prepare_MLPnPRansacBatch(host_prs, diag=False)
        got, want = call(), mt.prepare_MLPnPRansacBatch(host_prs, host=True, diag=False)()
        for g, w in zip(got, want):   # the same bits, or the figures below compare different things
            assert g["found"] == w["found"] and g["iterations_run"] == w["iterations_run"] and g["Tcw"].tobytes() == w["Tcw"].tobytes()
            assert np.array_equal(g["inlier"], w["inlier"]) and g["best_inliers"] == w["best_inliers"]
        res_call = mt.prepare_MLPnPRansacBatch(problems(B, n_hyp, min_inliers, True), diag=False)
        for g, w in zip(res_call(), want):
            assert g["Tcw"].tobytes() == w["Tcw"].tobytes() and g["best_inliers"] == w["best_inliers"]
        wall = timed(call.c_call, calls)
        wall_res = timed(res_call.c_call, calls)
        host = timed(call.c_call_host, max(10, calls // 10), warm=3)
        mt.profile(True)
        for _ in range(20):
            call.c_call()
        prof = mt.profile_read()
        mt.profile(False)
        kern = {k: round(prof[k][0] / max(prof[k][1], 1) * 1e3, 1) for k in ("k_mlpnp_hypotheses", "k_mlpnp_select")}
        return dict(N=args.n, hypotheses=n_hyp, problems=B, min_inliers=min_inliers, found=[g["found"] for g in got][:4],
                    iterations_run=[g["iterations_run"] for g in got][:4], refines=[g["refines"] for g in got][:4],
                    call_host_arrays=wall, call_resident=wall_res, kernel_event_us=kern, host_build_one_core=host)

    pool = F.MapPointPool(16 * args.n, lib=lib)
    batches = [int(v) for v in args.batches.split(",") if v]
    result = dict(what="MLPnPsolver, every hypothesis of a call at once; synchronous; %d calls after 20 warm-up calls.  "
                       "host_build_one_core is this project's restatement (csrc/mlpnp_math.h compiled for the host), NOT the "
                       "reference's MLPnPsolver, which needs Eigen and was not built" % args.calls)
    result["run_through"] = {str(B): measure(B, 35, args.n, args.calls) for B in batches}
    result["early_stop"] = {str(B): measure(B, 35, args.n // 2, args.calls) for B in batches}
    result["run_through_300"] = {"1": measure(1, 300, args.n, max(50, args.calls // 3))}
    for fr in keep:
        fr.close()
    pool.close()
    mt.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": result}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
