"""Per-call latency of Optimizer::PoseOptimization (src/Optimizer.cc:814-1114) at KITTI size - 2 000 features, the frame and the
map points resident on the device - in three settings:

    motion_model   about 300 of the features matched (Tracking::TrackWithMotionModel, Tracking.cc:2943)
    local_map      about 1 200 matched (Tracking::TrackLocalMap, :3005 / :3011)
    batch          B = 1, 16, 256 independent frames of the motion-model kind in one launch (rgbl_pose_optimization_batch)

For each: the wall time of the C call (time.perf_counter around the prepared ctypes call: host pointers in, host arrays out,
synchronous), its kernel time (the handle's HIP-event profile, a separate set of calls), and beside it the HOST build of
csrc/poseopt_math.h on one core (rgbl_pose_optimization_host on the same frames, host arrays; per frame on the first 8 frames
of a batch, multiplied out for all_frames_us).  That host figure is THIS
PROJECT'S restatement, not g2o: nobody has measured g2o for this function on this machine, and no speed-up against the
reference follows from these numbers.

    python tools/pose_opt_bench.py [--n 2000] [--calls 200] [--out profiles/pose_opt_calls.json]      on the MI355X

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
from orb_slam3_rgbl_amd import cases  # noqa: E402


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
    pool = F.MapPointPool(1 << 19, lib=lib)
    frames, next_slot = [], [0]

    def resident(case):
        """the frame on the device, its map points in slots of the shared pool"""
        n = len(case["mp_index"])
        fr = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), case["xy"], case["octave"], case["uright"])
        frames.append(fr)
        slot = np.arange(next_slot[0], next_slot[0] + len(case["world_pos"]), dtype=np.int32)
        next_slot[0] += len(slot)
        pool.update(slot, world_pos=case["world_pos"])
        keep = {k: case[k] for k in ("mp_index", "q", "t", "K", "bf", "inv_level_sigma2", "n_levels")}
        return dict(keep, device=fr, pool=pool, slot=slot)

    def measure(host_cases, calls):
        B = len(host_cases)
        dev = [resident(c) for c in host_cases]
        call = mt.prepare_PoseOptimizationBatch(dev)
        host = mt.prepare_PoseOptimizationBatch(host_cases, host=True)
        got, want = call(), host()
        for g, w in zip(got, want):   # the same bits, or the figures below compare different things
            assert g["result"] == w["result"] and np.array_equal(g["outlier"], w["outlier"]) and g["q64"].tobytes() == w["q64"].tobytes()
        wall = timed(call.c_call, calls)
        mt.profile(True)
        for _ in range(20):
            call.c_call()
        ms, cnt = mt.profile_read()["k_pose_opt"]
        mt.profile(False)
        host_one = [mt.prepare_PoseOptimizationBatch([c], host=True) for c in host_cases[:8]]   # per frame: the python glue stays out
        per_frame = [timed(h1, max(5, calls // 8), warm=2)["median_us"] for h1 in host_one]
        host_wall = dict(median_us_per_frame=round(float(np.median(per_frame)), 1), all_frames_us=round(float(np.mean(per_frame)) * B, 1))
        return dict(problems=B, matched=[int((c["mp_index"] >= 0).sum()) for c in host_cases][:4], inliers=[g["result"] for g in got][:4],
                    levenberg_iterations=[int(g["iterations"].sum()) for g in got][:4],
                    call=wall, kernel_us=round(ms / max(cnt, 1) * 1e3, 1), host_build_one_core=host_wall)

    result = dict(what="Optimizer::PoseOptimization, %d features, frame and map points resident, host arrays out, synchronous; "
                       "median of %d calls.  host_build_one_core is this project's restatement (csrc/poseopt_math.h compiled for the "
                       "host), NOT g2o" % (args.n, args.calls), n=args.n)
    result["motion_model"] = measure([cases.make_pose_opt_case(args.n, 300, seed=3)], args.calls)
    result["local_map"] = measure([cases.make_pose_opt_case(args.n, 1200, seed=11)], args.calls)
    result["batch"] = {str(B): measure([cases.make_pose_opt_case(args.n, 300, seed=100 + b) for b in range(B)], max(20, args.calls // max(1, B // 8)))
                       for B in (1, 16, 256)}
    mt.close()
    for f in frames:
        f.close()
    pool.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": result}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
