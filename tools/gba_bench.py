"""Per-call latency and the kernel split of Optimizer::BundleAdjustment's optimize(nIterations) (src/Optimizer.cc:52-390) through
rgbl_bundle_adjustment - ONE problem spread over the device, the reduced camera system factorised in panels (csrc/gba.hip) - at

    30 + 30 key frames /   3 000 points   lba_cases.local_mapping_case's scene, with rgbl_local_bundle_adjustment's own
                                          figure from the same run beside it (the same vertices and edges)
    200 key frames     /  20 000 points
    1 000 key frames   / 100 000 points

host arrays in, host arrays out, robust, 10 iterations.  The wall time of the C call (time.perf_counter around the prepared
ctypes call, synchronous; warm-up calls, then the median, minimum and 90th percentile), the time per kernel (the matcher's
HIP-event profile, a separate set of calls) and, where it ends in seconds, the HOST build on one core.  That host figure is THIS
PROJECT'S restatement (csrc/lba_math.h with lm_solve_panel compiled for the host), not g2o: g2o cannot be built here (no Eigen),
and no speed-up against the reference follows from these numbers.

--ab measures the panel width instead: the factorisation and substitution kernels at n = 768 and n = 6 144 unknowns for
RGBL_GBA_PANEL = 16, 32 and 64, each width in a fresh process (the switch is read once, when the matcher is created).

    python tools/gba_bench.py [--calls 10] [--ab] [--out profiles/gba_calls.json]      on the MI355X

One JSON line on stdout; --out writes (or, with --ab, extends) the file.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_rgbl_amd import lba_cases as lc  # noqa: E402

SOLVE = ("k_gba_trailing", "k_gba_diag", "k_gba_rows", "k_gba_start", "k_gba_forward", "k_gba_scale", "k_gba_backward", "k_gba_finish")


def stats(t):
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def timed(call, calls, warm):
    t = []
    for _ in range(calls + warm):
        a = time.perf_counter()
        call()
        t.append((time.perf_counter() - a) * 1e6)
    return stats(t[warm:])


def profiled(mt, call, n_prof):
    mt.profile(True)   # resets the totals
    for _ in range(n_prof):
        call()
    k = {name: dict(us_per_call=round(ms / n_prof * 1e3, 1), launches_per_call=cnt // n_prof) for name, (ms, cnt) in mt.profile_read().items()
         if (name.startswith("k_lba") or name.startswith("k_gba")) and cnt > 0}   # the timer keeps the names of earlier sets: no empty rows
    mt.profile(False)
    return k


def scene(n_cams, n_fixed, n_points, step=0.4, max_iterations=10):
    return lc.make_ba_case(n_cams=n_cams, n_fixed=n_fixed, n_points=n_points, obs_per_point=(3, 7), seed=5, outlier_share=0.02,
                           step=step, max_iterations=max_iterations)


def measure(mt, lib, F, case, calls, host):
    dev = mt.prepare_BundleAdjustment(case)
    got = dev()
    r = dict(cams=int(case["n_cams"]), fixed=int(case["cam_is_fixed"].sum()), points=len(case["world_pos"]), edges=len(case["edge_point"]),
             active_cams=int(got["active_cams"]), unknowns_reduced=6 * int(got["active_cams"]), iterations=int(got["iterations"]),
             trials=int(got["trials"]), rejected=int(got["rejected"]), failed=int(got["failed"]), first_chi2=got["first_chi2"],
             last_chi2=got["last_chi2"])
    if host:
        hc = F.bundle_adjustment_call(lib, None, case)
        a = time.perf_counter()
        want = hc()
        r["host_build_one_core_us"] = round((time.perf_counter() - a) * 1e6, 1)   # one call: it takes long
        for k in ("cam_q", "cam_t", "point", "chi2"):   # the same bits, or the figures compare different things
            assert got[k].tobytes() == want[k].tobytes(), k
    r["call"] = timed(dev, calls, 2)
    r["kernels"] = profiled(mt, dev, 3)
    r["kernel_us_per_call"] = round(sum(v["us_per_call"] for v in r["kernels"].values()), 1)
    r["solve_us_per_trial"] = round(sum(v["us_per_call"] for k, v in r["kernels"].items() if k in SOLVE) / max(1, r["trials"]), 1)
    return r


def run_sizes(args):
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)
    out = dict(what="Optimizer::BundleAdjustment's optimize(10), robust, host arrays in and out, synchronous; median of %d calls after 2 "
                    "warm-up calls.  host_build_one_core is this project's restatement compiled for the host (ONE call), NOT g2o" % args.calls,
               panel=int(os.environ.get("RGBL_GBA_PANEL", "32")))
    small = scene(60, 30, 3000)
    out["kf30+30_pts3000"] = measure(mt, lib, F, small, args.calls, True)
    # LocalBundleAdjustment on the same vertices and edges, in the same run
    lba_case = lc.as_lba_case(small)
    lba = mt.prepare_LocalBundleAdjustment(lba_case)
    got = lba()
    k = profiled(mt, lba, 3)
    out["kf30+30_pts3000"]["local_bundle_adjustment"] = dict(
        trials=int(got["trials"]), iterations=int(got["iterations"]), call=timed(lba, args.calls, 2), kernels=k,
        k_lba_factor_us_per_trial=round(k["k_lba_factor"]["us_per_call"] / max(1, int(got["trials"])), 1))
    out["kf200_pts20000"] = measure(mt, lib, F, scene(200, 1, 20000, step=0.1), max(3, args.calls // 2), True)
    out["kf1000_pts100000"] = measure(mt, lib, F, scene(1000, 1, 100000, step=0.02), 3, False)   # the host build is cubic: not run
    mt.close()
    return out


def run_width(args):
    """one width (this process's RGBL_GBA_PANEL): the solve kernels at n = 768 and n = 6 144, one iteration each"""
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    mt = F.ORBmatcher(0.6, False, lib=lib)
    out = {}
    for name, nA, pts in (("n768", 128, 4000), ("n6144", 1024, 20000)):
        case = scene(nA + 1, 1, pts, step=0.02, max_iterations=1)
        dev = mt.prepare_BundleAdjustment(case)
        got = dev()
        assert got["active_cams"] == nA and got["failed"] == 0
        k = profiled(mt, dev, 3)
        out[name] = dict(trials=int(got["trials"]), us_per_trial={n: round(k[n]["us_per_call"] / got["trials"], 1) for n in SOLVE if n in k},
                         solve_us_per_trial=round(sum(k[n]["us_per_call"] for n in SOLVE if n in k) / got["trials"], 1))
    mt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--width", action="store_true", help="(internal) one width of --ab, in this process")
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    if args.width:
        print(json.dumps(run_width(args)))
        return
    if args.ab:
        result = {}
        for w in (16, 32, 64):   # a fresh process per width, one after the other
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--width"], env=dict(os.environ, RGBL_GBA_PANEL=str(w)),
                                 capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.stderr.write(res.stdout[-2000:] + res.stderr[-2000:])
                sys.exit(res.returncode)
            result["panel_%d" % w] = json.loads(res.stdout.strip().splitlines()[-1])
        result = {"panel_width": result}
    else:
        result = {"device": run_sizes(args)}
    print(json.dumps(result))
    if args.out:
        old = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        old.update(result)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
