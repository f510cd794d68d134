"""Per-call latency of TwoViewReconstruction (src/TwoViewReconstruction.cc) on the device - every homography and fundamental
hypothesis of a call at once - at the size Tracking::MonocularInitialization calls it: 2 000 keys per frame, 200 hypotheses
(Pinhole.cpp:87), N = 100, 300 and 1 000 matches, on a general scene (the fundamental path) and on a planar one in which every
set is the same doubled one - four points twice, on which the fundamental system has rank 4 - so that the homography wins and
ReconstructH's eight motion hypotheses run (with sets drawn at random a planar scene goes the fundamental way here: SF >= SH).

Forms: host arrays in and out, and resident frames (two DeviceFrames: only the matches and the sets travel).  For each: the wall
time of the C call (time.perf_counter around the prepared ctypes call, which ends in a stream synchronise), warmed up, median /
min / p10 / p90 over --calls repetitions; the kernels' times from the handle's HIP-event profile (a separate set of calls); and
beside it the HOST build of csrc/twoview_math.h on one core (rgbl_two_view_reconstruct_host on the same problems).  That host
figure is THIS PROJECT'S restatement, not the reference: the reference's TwoViewReconstruction needs Eigen and OpenCV and has
not been built or measured here, and no speed-up against it follows from these numbers.

    python tools/two_view_bench.py [--keys 2000] [--calls 200] [--out profiles/two_view_calls.json]      on the MI355X

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
from orb_slam3_rgbl_amd import twoview_cases as tc  # noqa: E402

KERNELS = ("k_tv_normalize", "k_tv_hypotheses", "k_tv_select", "k_tv_check_rt", "k_tv_decide")


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
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=200)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--matches", default="100,300,1000")
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

    def problem(N, scene):
        case = tc.make_two_view_case(N, args.hyp, seed=70 + N, scene=scene, pixel_noise=0.1, outlier_share=0.0 if scene == "planar" else 0.2,
                                     extra1=args.keys - N, extra2=args.keys - N)
        pr = tc.problem(case)
        if scene == "planar":   # four points twice in every set: F fits little, H wins (tests/twoview_checks.py: doubled)
            first, second = tc.matches(case)
            xy1, xy2, s = case["xy1"].copy(), case["xy2"].copy(), case["samples"].copy()
            at = (3, 30, 60, 90)
            for p in at:
                xy1[first[p + 1]], xy2[second[p + 1]] = xy1[first[p]], xy2[second[p]]
            s[:] = [q for p in at for q in (p, p + 1)]
            pr = dict(pr, xy1=xy1, xy2=xy2, samples=s)
        return pr

    def measure(N, scene):
        pr = problem(N, scene)
        call = mt.prepare_TwoViewReconstructBatch([pr], diag=False)
        got, want = call()[0], mt.prepare_TwoViewReconstructBatch([pr], host=True, diag=False)()[0]
        for k in ("found", "model", "exit_code", "best_h", "best_f", "n_inliers", "best_motion"):   # the same bits, or the figures compare different things
            assert got[k] == want[k], (k, got[k], want[k])
        assert got["R21"].tobytes() == want["R21"].tobytes() and got["p3d"].tobytes() == want["p3d"].tobytes() and np.array_equal(got["n_good"], want["n_good"])
        fr1 = F.DeviceFrame(args.keys, lib=lib).upload(np.zeros((args.keys, 32), np.uint8), pr["xy1"], np.zeros(args.keys, np.int32), np.full(args.keys, -1, np.float32))
        fr2 = F.DeviceFrame(args.keys, lib=lib).upload(np.zeros((args.keys, 32), np.uint8), pr["xy2"], np.zeros(args.keys, np.int32), np.full(args.keys, -1, np.float32))
        keep.extend([fr1, fr2])
        res = {k: v for k, v in pr.items() if k not in ("xy1", "xy2")}
        res_call = mt.prepare_TwoViewReconstructBatch([dict(res, n1=args.keys, n2=args.keys, device1=fr1, device2=fr2)], diag=False)
        g = res_call()[0]
        assert g["R21"].tobytes() == want["R21"].tobytes() and g["found"] == want["found"]
        wall = timed(call.c_call, args.calls)
        wall_res = timed(res_call.c_call, args.calls)
        host = timed(call.c_call_host, max(10, args.calls // 10), warm=3)
        mt.profile(True)
        for _ in range(20):
            call.c_call()
        prof = mt.profile_read()
        mt.profile(False)
        kern = {k: round(prof[k][0] / max(prof[k][1], 1) * 1e3, 1) for k in KERNELS}
        return dict(matches=N, keys=args.keys, hypotheses=args.hyp, scene=scene, model=got["model"], found=got["found"], exit_code=got["exit_code"],
                    n_inliers=got["n_inliers"], call_host_arrays=wall, call_resident=wall_res, kernel_event_us=kern, host_build_one_core=host)

    result = dict(what="TwoViewReconstruction, every hypothesis of a call at once; synchronous; %d calls after 20 warm-up calls.  "
                       "host_build_one_core is this project's restatement (csrc/twoview_math.h compiled for the host), NOT the "
                       "reference's TwoViewReconstruction, which needs Eigen and was not built" % args.calls)
    for scene, key in (("general", "fundamental"), ("planar", "homography")):
        result[key] = {v: measure(int(v), scene) for v in args.matches.split(",") if v}
    for fr in keep:
        fr.close()
    mt.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": result}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
