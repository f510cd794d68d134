"""Per-call latency of LocalMapping::CreateNewMapPoints' neighbour loop (src/LocalMapping.cc:434-711) for a key frame of KITTI
size - 2 000 features, 10 neighbours, resident frames - two ways in the same run:

    one_call    rgbl_create_new_map_points: every search and every per-match block chained on the matcher's stream, one upload,
                one read-back
    parent      what the tree did before: rgbl_search_triangulation once per neighbour that is searched (8 of the 10: one is
                closer than mb, one left out by skip[]), the per-match block on the host between two calls (csrc/newpoint_math.h's
                host build, rgbl_triangulate_matches_host) and the has_mappoint feedback - frontend's restatement with these two
                plugged in.  c_calls_us sums the time inside the C calls alone; wall_us includes the numpy glue between them

    python tools/new_points_bench.py [--n 2000] [--neighbours 10] [--calls 200] [--out profiles/new_points_calls.json]   on the MI355X

    python tools/new_points_bench.py --cpu-reference [--out ...]      where the reference sources are: the reference's own
                LocalMapping::CreateNewMapPoints on the same case (tests/new_points_golden.py cuts it out and compiles it unmodified,
                -O2, one thread, its SearchForTriangulation the reference's ORBmatcher.cc; timed around the glue call, which builds the
                stand-in KeyFrame objects and flattens them again for every search, and whose SVD is the header's, not Eigen's)

Only the calls are timed (time.perf_counter, host arrays in, host arrays out, synchronous); the median of --calls calls is
reported, kernel times come from the handle's HIP-event profile in a separate set of calls.  One JSON line on stdout; --out
merges the result into a JSON file under its mode's key.
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


def stats(t):
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def write(args, key, result):
    print(json.dumps({key: result}))
    if args.out:
        merged = {}
        if os.path.exists(args.out):
            with open(args.out) as fh:
                merged = json.load(fh)
        merged[key] = result
        with open(args.out, "w") as fh:
            json.dump(merged, fh, indent=1)
            fh.write("\n")


def cpu_reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import new_points_golden as ng
    lib = ng.build_reference_glue()
    ng.CASES["bench"] = dict(n=args.n, n_neigh=args.neighbours, seed=5)
    case = ng.make_case("bench", ng.reference_geometry(lib, ng.make_case("bench", None)))
    case["skip"][:] = cases.make_new_points_case(args.n, args.neighbours, seed=5)["skip"]   # not expressible in the reference: see below
    skipped = [i for i in range(args.neighbours) if case["skip"][i]]
    for i in skipped:   # the device rows leave this neighbour out through skip[]; here every feature of it holds a map point
        kf = case["neighbours"][i]["kf"]
        kf["has_mp"] = np.ones_like(kf["has_mp"])
    call = ng.reference_results(lib, "bench", case, prepare=True)
    rec = call()
    calls = max(10, args.calls // 10)
    t = []
    for _ in range(calls + 2):
        a = time.perf_counter()
        call()
        t.append((time.perf_counter() - a) * 1e6)
    cpu = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")][:1]
    write(args, "cpu_reference", dict(
        what="the reference's own LocalMapping::CreateNewMapPoints (cut out of src/LocalMapping.cc, compiled unmodified, -O2, one thread) with the "
             "reference's ORBmatcher::SearchForTriangulation, on the device rows' case with the reference's pose arithmetic; timed around the glue "
             "call, which builds the stand-in objects; the neighbour the device rows leave out through skip[] has every feature taken",
        n=args.n, neighbours=args.neighbours, new_points=int(len(rec)), host_cpu=cpu[0] if cpu else "", calls=calls, call=stats(t[2:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--cpu-reference", action="store_true")
    args = ap.parse_args()
    if args.cpu_reference:
        return cpu_reference(args)
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    case = cases.make_new_points_case(args.n, args.neighbours, seed=5, report_rejected=0)
    frames = []

    def res(kf):
        f = F.DeviceFrame(len(kf["desc"]), lib=lib)
        f.upload(kf["desc"], kf["xy"], kf["octave"], kf["uright"])
        f.set_feature_vector(kf["node_off"], kf["node_feat"])
        frames.append(f)
        return dict(kf, device=f)
    kf1 = res(case["kf1"])
    neigh = [dict(nb, kf=res(nb["kf"])) for nb in case["neighbours"]]
    prm, skip = case["prm"], case["skip"]
    mt = F.ORBmatcher(0.6, False, lib=lib)

    # one call
    one = mt.prepare_CreateNewMapPoints(kf1, neigh, prm, skip)
    recs, per, mask = one()
    want = (recs.copy(), per.copy(), mask.copy())
    t = []
    for i in range(args.calls + 10):
        a = time.perf_counter()
        one()
        t.append((time.perf_counter() - a) * 1e6)
    one_call = stats(t[10:])
    mt.profile(True)
    for _ in range(50):
        one()
    prof = mt.profile_read()
    mt.profile(False)
    kern = {name: dict(per_launch_us=round(ms / max(cnt, 1) * 1e3, 1), launches_per_call=cnt // 50, per_call_us=round(ms / 50 * 1e3, 1))
            for name, (ms, cnt) in prof.items()}

    # the parent path: frontend's restatement with the device's single-call search and the header's host block, both timed
    runs = [i for i in range(len(neigh)) if per[i] >= 0]
    live = {i: np.zeros(args.n, np.uint8) for i in runs}   # shared with the prepared searches, rewritten in place
    searches = {i: mt.prepare_SearchForTriangulation(dict(kf1, has_mp=live[i]), neigh[i]["kf"], neigh[i]["F12"], neigh[i]["ep"],
                                                     neigh[i]["kf"]["scale_factors"], neigh[i]["kf"]["level_sigma2"], False, False) for i in runs}
    index_of = {id(nb): i for i, nb in enumerate(neigh)}
    keep = []
    k1s = F.ORBmatcher._new_points_kf(case["kf1"], keep)
    k2s = {i: F.ORBmatcher._new_points_kf(case["neighbours"][i]["kf"], keep) for i in runs}
    P = F.ORBmatcher._new_points_params(dict(prm, report_rejected=1))
    out = np.zeros(args.n, L.NEW_POINT_DTYPE)
    inside_c = [0.0]

    def search(k1, nb):
        i = index_of[id(nb)]
        live[i][:] = k1["has_mp"]
        a = time.perf_counter()
        m12 = searches[i]()[2]
        inside_c[0] += time.perf_counter() - a
        return m12

    def block(i, idx1, idx2):
        a = time.perf_counter()
        lib.rgbl_triangulate_matches_host(C.byref(k1s), C.byref(k2s[i]), C.byref(P), len(idx1), L.ptr(idx1), L.ptr(idx2), L.ptr(out))
        inside_c[0] += time.perf_counter() - a
        return out[:len(idx1)]

    def parent():
        inside_c[0] = 0.0
        got, _, mask_after = mt.CreateNewMapPointsRestatement(search, kf1, neigh, prm, skip, block=block)
        live_mask[:] = mask_after
        return inside_c[0] * 1e6, got
    live_mask = np.zeros(args.n, np.uint8)
    _, got = parent()
    assert got.tobytes() == want[0].tobytes() and np.array_equal(live_mask, want[2]), "the parent path and the one call differ"
    wall, inside = [], []
    for i in range(args.calls + 10):
        a = time.perf_counter()
        c_us, _ = parent()
        wall.append((time.perf_counter() - a) * 1e6)
        inside.append(c_us)
    result = dict(what="LocalMapping::CreateNewMapPoints' neighbour loop, resident frames, host arrays out, synchronous; median of %d calls" % args.calls,
                  n=args.n, neighbours=args.neighbours, neighbours_searched=len(runs), matches=int(per[per > 0].sum()), new_points=int(len(recs)),
                  one_call=dict(call=one_call, kernels=kern, kernels_total_us=round(sum(k["per_call_us"] for k in kern.values()), 1)),
                  parent=dict(c_calls_us=stats(inside[10:]), wall_us=stats(wall[10:])))
    result["parent_c_calls_over_one_call"] = round(result["parent"]["c_calls_us"]["median_us"] / one_call["median_us"], 2)
    mt.close()
    for f in frames:
        f.close()
    write(args, "device", result)


if __name__ == "__main__":
    main()
