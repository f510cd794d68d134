"""Per-call latency of refreshing map points - MapPoint::UpdateNormalAndDepth + MapPoint::ComputeDistinctiveDescriptors - to the
same pool state, two ways, on maps of 40 key frames with 2 000 features each and about 15 observations per point:

    parent   what a host did before rgbl_map_points_refresh: gather every observation's descriptor row out of the key frames'
             host matrices (here one numpy fancy index over precomputed row numbers), rgbl_distinctive_descriptors on them
             (32 bytes per observation go up), copy the winning rows, rgbl_map_points_update with all five arrays (68 bytes
             per point).  The host's own normal / distance arithmetic is NOT in the timed part (its results are precomputed),
             which favours this row.
    refresh  rgbl_map_points_refresh: 8 bytes per observation and 32 per point go up (slot, offset, position, reference key
             frame and level), the descriptors are read from the resident key frames, one synchronisation

    python tools/map_refresh_bench.py [--points 1500 300 5000] [--calls 300] [--out profiles/map_refresh_calls.json]     on the MI355X

Only the calls themselves are timed (time.perf_counter around them, host arrays in, host arrays out, synchronous); median /
min / p90 of --calls calls, the parent path twice to show the spread between two runs; kernel times come from the matcher
handle's HIP-event profile in a separate 50 calls (the scatter kernel of rgbl_map_points_update runs on the pool's own stream
and is not in them).  One JSON line on stdout; --out writes the same document."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_rgbl_amd import cases  # noqa: E402


def stats_us(fn, calls, warmup=10):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e6)
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def staged(*array_bytes):
    return sum((b + 255) // 256 * 256 for b in array_bytes)


def kernels(mt, fn):
    mt.profile(True)
    for _ in range(50):
        fn()
    prof = mt.profile_read()
    mt.profile(False)
    k = {name: round(ms / max(cnt, 1) * 1e3, 1) for name, (ms, cnt) in prof.items()}
    return k, round(sum(k.values()), 1)


def bench_case(lib, L, F, n_points, calls, profile):
    case = cases.make_map_refresh_case(n_points, 40, seed=5, features=2000)
    n = len(case["slot"])
    frames = [F.DeviceFrame(len(d), lib=lib).upload(d, xy, o) for d, xy, o in zip(case["kf_desc"], case["kf_xy"], case["kf_octave"])]
    start = np.concatenate([[0], np.cumsum(case["kf_n"])]).astype(np.int64)
    table = np.concatenate(case["kf_desc"])
    good = case["kf_bad"][case["obs_kf"]] == 0
    row_index = (start[case["obs_kf"]] + case["obs_feat"])[good]
    rows_per_point = np.add.reduceat(np.concatenate([good, [False]]).astype(np.int64), case["obs_off"][:-1].astype(np.int64)) * (np.diff(case["obs_off"]) > 0)
    off_good = np.concatenate([[0], np.cumsum(rows_per_point)]).astype(np.int32)
    has = rows_per_point > 0
    fill = (case["slot"], case["world_pos"], case["normal0"], case["min_dist0"], case["max_dist0"], case["desc0"])

    # the new call, once, for the values the parent path's host would have computed itself
    pool_new = F.MapPointPool(n, lib=lib)
    pool_new.update(*fill)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    refresh = pool_new.prepare_refresh(mt, dict(case, kf_frames=frames, new_world_pos=case["world_pos"]))
    got = {k: v.copy() for k, v in refresh().items()}

    # the parent path
    pool_old = F.MapPointPool(n, lib=lib)
    pool_old.update(*fill)
    mt_old = F.ORBmatcher(0.8, True, lib=lib)
    best = np.zeros(n, np.int32)
    desc_new = case["desc0"].copy()
    fn, h = lib.rgbl_distinctive_descriptors, mt_old.h

    def parent():
        rows = table[row_index]                                              # the host's gather
        L.check(lib, fn(h, L.ptr(rows), L.ptr(off_good), n, L.ptr(best)))
        desc_new[has] = rows[off_good[:-1][has] + best[has]]                 # mDescriptor = vDescriptors[BestIdx].clone()
        pool_old.update(case["slot"], case["world_pos"], got["normal"], got["min_dist"], got["max_dist"], desc_new)
    parent()
    a, b = pool_old.download(case["slot"]), pool_new.download(case["slot"])
    same = all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) or
               (a[k].dtype == np.float32 and bool(np.all((a[k].view(np.uint32) == b[k].view(np.uint32)) | (np.isnan(a[k]) & np.isnan(b[k])))))
               for k in a)
    n_obs, n_rows = int(case["obs_off"][-1]), int(off_good[-1])
    r = dict(points=n, key_frames=40, features_per_key_frame=2000, observations=n_obs, descriptor_rows=n_rows,
             pool_state="refresh leaves the pool as the parent path does" if same else "MISMATCH")
    r["parent_run1"] = stats_us(parent, calls)
    r["refresh"] = stats_us(refresh, calls)
    r["parent_run2"] = stats_us(parent, calls)
    r["refresh_run2"] = stats_us(refresh, calls)
    # what each path copies to the device per call: the arrays it stages, each padded to the arenas' 256-byte alignment
    n_kfs, n_levels = len(case["kf_n"]), len(case["scale_factors"])
    r["parent_upload_bytes"] = staged(32 * n_rows, 4 * (n + 1)) + staged(4 * n, 12 * n, 12 * n, 4 * n, 4 * n, 32 * n)
    r["refresh_upload_bytes"] = staged(4 * n, 4 * (n + 1), 12 * n, 4 * n_obs, 4 * n, 4 * n, 12 * n_kfs, 4 * n_levels,   # slot, offsets, positions, obs_kf, ref_kf, ref_level, centres, scales
                                       4 * n_obs, 4 * n, n_kfs, 8 * n_kfs)                                             # obs_feat, long-list offsets, bad flags, descriptor pointers
    if profile:
        r["parent_kernels_us"], r["parent_kernels_total_us"] = kernels(mt_old, parent)
        r["refresh_kernels_us"], r["refresh_kernels_total_us"] = kernels(mt, refresh)
    spread = abs(r["parent_run1"]["median_us"] - r["parent_run2"]["median_us"])
    gain = min(r["parent_run1"]["median_us"], r["parent_run2"]["median_us"]) - max(r["refresh"]["median_us"], r["refresh_run2"]["median_us"])
    r["parent_spread_us"], r["gain_us"] = round(spread, 1), round(gain, 1)
    r["refresh_wins_by_more_than_the_spread"] = bool(gain > spread)
    for x in [pool_new, pool_old, mt, mt_old] + frames:
        x.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[1500, 300, 5000])
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    doc = dict(what="MapPoint::UpdateNormalAndDepth + ComputeDistinctiveDescriptors to the same pool state: host gather + "
                    "rgbl_distinctive_descriptors + rgbl_map_points_update (parent; the host's normal arithmetic not timed) against "
                    "rgbl_map_points_refresh; median / min / p90 of %d synchronous calls, the runs interleaved parent, refresh, parent, "
                    "refresh; kernels_us from HIP events on the matcher's stream in 50 further calls" % args.calls,
               date=time.strftime("%Y-%m-%d"))
    for n in args.points:
        doc["points_%d" % n] = bench_case(lib, L, F, n, args.calls, not args.no_profile)
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
