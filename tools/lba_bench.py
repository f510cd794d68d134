"""Per-call latency of Optimizer::LocalBundleAdjustment from :1188 on (src/Optimizer.cc) at a local-mapping shape - 30 free
and 30 fixed key frames, 3 000 points, about 5 observations per point (lba_cases.local_mapping_case), host arrays in, host
arrays out - through rgbl_local_bundle_adjustment: ONE problem spread over the device, Levenberg's loop on the host between
launches.

The wall time of the C call (time.perf_counter around the prepared ctypes call, synchronous; 3 warm-up calls, then the median,
minimum and 90th percentile of --calls calls), the time per kernel (the matcher's HIP-event profile, a separate set of calls)
and beside it the HOST build of csrc/lba_math.h on one core (rgbl_local_bundle_adjustment_host on the same problem).  That host
figure is THIS PROJECT'S restatement, not g2o: g2o cannot be built here (no Eigen), nobody has measured it for this function
on this machine, and no speed-up against the reference follows from these numbers.

    python tools/lba_bench.py [--calls 30] [--out profiles/lba_calls.json]      on the MI355X

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
from orb_slam3_rgbl_amd import lba_cases as lc  # noqa: E402


def stats(t):
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call, calls, warm=3):
    t = []
    for _ in range(calls + warm):
        a = time.perf_counter()
        call()
        t.append((time.perf_counter() - a) * 1e6)
    return stats(t[warm:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)
    case = lc.local_mapping_case()
    dev, host = mt.prepare_LocalBundleAdjustment(case), F.local_bundle_adjustment_call(lib, None, case)
    got, want = dev(), host()
    for k in ("cam_q", "cam_t", "point", "chi2", "flags"):   # the same bits, or the figures below compare different things
        assert got[k].tobytes() == want[k].tobytes(), k
    wall = timed(dev, args.calls)
    mt.profile(True)
    n_prof = 5
    for _ in range(n_prof):
        dev()
    kernels = {k: dict(us_per_call=round(ms / n_prof * 1e3, 1), launches_per_call=cnt // n_prof)
               for k, (ms, cnt) in mt.profile_read().items() if k.startswith("k_lba")}
    mt.profile(False)
    result = dict(what="Optimizer::LocalBundleAdjustment from :1188 on, host arrays in and out, synchronous; median of %d calls after 3 "
                       "warm-up calls.  host_build_one_core is this project's restatement (csrc/lba_math.h compiled for the host), "
                       "NOT g2o" % args.calls,
                  free=int(case["n_free"]), fixed=int(case["n_fixed"]), points=len(case["world_pos"]), edges=len(case["edge_point"]),
                  iterations=int(got["iterations"]), trials=int(got["trials"]), rejected=int(got["rejected"]),
                  erased=int((got["flags"] & 1).sum()), first_chi2=got["first_chi2"], last_chi2=got["last_chi2"],
                  call=wall, kernels=kernels, kernel_us_per_call=round(sum(v["us_per_call"] for v in kernels.values()), 1),
                  host_build_one_core=timed(host, max(5, args.calls // 3), warm=1))
    mt.close()
    print(json.dumps({"device": result}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": result}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
