"""Per-call latency of Tracking::SearchLocalPoints' second half (the isInFrustum loop + ORBmatcher::SearchByProjection) for a
local map of 3 000 points against a 2 000-feature frame, three ways:

    parent      what the tree did before rgbl_track_local_points: the loop on the host (here its numpy restatement,
                frontend.frustum_restatement - a Python cost; the C++ loop's own time is the --cpu-reference row) and
                rgbl_search_local_points on what it left
    host_arrays rgbl_track_local_points with the map points as host arrays (about 70 bytes per point go up with every call)
    pool        rgbl_track_local_points with the map points in a device-resident pool (6 bytes per point go up: slot, consider1, mp_observed1)

    python tools/local_map_bench.py [--n1 3000] [--n2 2000] [--calls 300] [--out profiles/local_map_calls.json]     on the MI355X
    python tools/local_map_bench.py --cpu-reference [--out ...]                                                where the reference sources are

Only the call itself is timed (time.perf_counter around the ctypes call, host arrays in, host arrays out, synchronous); the
median of --calls calls is reported, kernel times come from the handle's HIP-event profile in a separate set of calls.
One JSON line on stdout; --out merges the result into a JSON file under its mode's key.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_rgbl_amd import cases  # noqa: E402

TH = 3.0


def median_us(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e6)
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def kernels(mt, fn):
    mt.profile(True)
    for _ in range(50):
        fn()
    prof = mt.profile_read()
    mt.profile(False)
    k = {name: round(ms / max(cnt, 1) * 1e3, 1) for name, (ms, cnt) in prof.items()}
    return k, round(sum(k.values()), 1)


def bench_gpu(args):
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    case = cases.make_local_map_case(args.n1, args.n2, seed=41)
    n1, n2 = len(case["world_pos1"]), len(case["kp2_xy"])
    out = dict(n1=n1, n2=n2, th=TH)
    rows = {}
    # the parent commit's path
    t0 = time.perf_counter()
    iv, rec, _ = F.frustum_restatement(case)
    loop_us = (time.perf_counter() - t0) * 1e6
    mt = F.ORBmatcher(0.8, True, lib=lib)
    search = mt.prepare_SearchLocalPoints(cases.local_points_from_cull(case, iv, rec), TH)
    want_m, want_n = [np.copy(v) if isinstance(v, np.ndarray) else v for v in search()]
    r = dict(call=median_us(search, args.calls), host_loop_numpy_us=round(loop_us, 1), upload_bytes_per_point=1 + 12 + 4 + 4 + 32 + 1)
    if not args.no_profile:
        r["kernels_us"], r["kernels_total_us"] = kernels(mt, search)
    rows["parent_search_local_points"] = r
    mt.close()
    out["in_view"], out["matches"] = int(iv.sum()), int(want_n)
    # the one-call forms
    pool = F.MapPointPool(n1, lib=lib)
    t0 = time.perf_counter()
    pool.update(np.arange(n1, dtype=np.int32), case["world_pos1"], case["normal1"], case["min_dist1"], case["max_dist1"], case["mp_desc1"])
    fill_us = (time.perf_counter() - t0) * 1e6
    hollow = {k: None for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1")}
    for name, c, per_point in (("track_host_arrays", case, 1 + 12 + 12 + 4 + 4 + 32 + 1),
                               ("track_pool", dict(case, pool=pool, slot1=np.arange(n1, dtype=np.int32), **hollow), 1 + 4 + 1)):
        mt = F.ORBmatcher(0.8, True, lib=lib)
        call = mt.prepare_TrackLocalPoints(c, TH)
        got = call()
        ok = got[2] == int(iv.sum()) and got[4] == want_n and np.array_equal(got[3], want_m) and np.array_equal(got[0], iv)
        r = dict(call=median_us(call, args.calls), upload_bytes_per_point=per_point, result="as the parent path" if ok else "MISMATCH")
        bare = mt.prepare_TrackLocalPoints(c, TH, records=False)
        r["call_without_records"] = median_us(bare, args.calls)
        if not args.no_profile:
            r["kernels_us"], r["kernels_total_us"] = kernels(mt, call)
        rows[name] = r
        mt.close()
    rows["track_pool"]["pool_fill_us"] = round(fill_us, 1)
    # a few percent of the local map change between frames: what an update of 100 points costs
    idx = np.arange(100, dtype=np.int32)
    a = [np.ascontiguousarray(case[k][:100]) for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1")]
    rows["pool_update_100_points"] = median_us(lambda: pool.update(idx, *a), args.calls)
    pool.close()
    return dict(what="rgbl_search_local_points on the restated loop's output (parent) / rgbl_track_local_points from host arrays / from "
                     "the pool: host arrays in, host arrays out, synchronous; median of %d calls; kernels_us from HIP events on the "
                     "matcher's stream" % args.calls, **out, **rows)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def bench_reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frustum_golden as fg
    from oracle import oracle_py as O
    from oracle import ref_py as R
    lib = fg.build_reference_glue()
    case = cases.make_local_map_case(args.n1, args.n2, seed=41)
    iv, rec = fg.reference_results(case, lib)
    n1 = len(case["world_pos1"])
    a = [np.ascontiguousarray(case[k], dt) for k, dt in (("consider1", np.uint8), ("world_pos1", np.float32), ("normal1", np.float32),
         ("min_dist1", np.float32), ("max_dist1", np.float32), ("Rcw", np.float32), ("tcw", np.float32), ("Ow", np.float32), ("K", np.float32))]
    a.append(np.ascontiguousarray(np.asarray(case["grid"], np.float32)[:4]))
    o = [np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros((n1, 5), np.float32), np.zeros(n1, np.int32)]
    argv = [n1] + [v.ctypes.data_as(C.c_void_p) for v in a] + [float(case["mbf"]), float(case["log_scale_factor"]), len(case["scale_factors"]),
                                                                float(case["viewing_cos_limit"])] + [v.ctypes.data_as(C.c_void_p) for v in o]
    t = []
    for k in range(args.calls + 3):
        t0 = time.perf_counter()
        lib.ref_frustum(*argv)
        if k >= 3:
            t.append((time.perf_counter() - t0) * 1e6)
    assert np.array_equal(o[0], iv)
    out = dict(n1=len(case["world_pos1"]), n2=len(case["kp2_xy"]), in_view=int(iv.sum()), host_cpu=cpu_model(),
               is_in_frustum_loop=dict(median_us=round(float(np.median(t)), 1), min_us=round(float(np.min(t)), 1), calls=len(t)))
    ref = R.load_matcher()
    if ref is not None:
        keep = []
        P = O.make_local_points_input(cases.local_points_from_cull(case, iv, rec), TH, 0.8, keep)
        ts = []
        for k in range(args.calls + 3):
            m, nm, sec = R.call_struct(ref, "ref_search_local_points", P, P.n2)
            if k >= 3:
                ts.append(sec * 1e6)
        out["search_by_projection"] = dict(median_us=round(float(np.median(ts)), 1), min_us=round(float(np.min(ts)), 1), matches=int(nm))
        out["sum_median_us"] = round(out["is_in_frustum_loop"]["median_us"] + out["search_by_projection"]["median_us"], 1)
    return dict(what="the reference's own Frame::isInFrustum + MapPoint::PredictScale lines (cut out of src/Frame.cc, src/MapPoint.cc, "
                     "compiled unmodified, -O2, one thread; timed around the glue call, which builds one MapPoint object per point) and "
                     "its ORBmatcher::SearchByProjection(F, vpMapPoints, ...) (oracle/_ref, timed inside the glue), same case as the device rows",
                **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=3000)
    ap.add_argument("--n2", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    key, res = ("cpu_reference", bench_reference(args)) if args.cpu_reference else ("device", bench_gpu(args))
    print(json.dumps({key: res}))
    if args.out:
        doc = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                doc = json.load(f)
        doc[key] = res
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
