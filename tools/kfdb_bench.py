"""Per-call latency of the KeyFrameDatabase query (rgbl_kfdb_query / rgbl_kfdb_query_batch) at several database sizes, and of
the reference's own DetectRelocalizationCandidates on one host core on the same inputs.

    python tools/kfdb_bench.py [--sizes 500,1500,5000] [--calls 200] [--out profiles/kfdb_calls.json]        on the MI355X
    python tools/kfdb_bench.py --cpu-reference [--calls 50] [--out ...]                                      where the reference sources are

Only the call itself is timed (time.perf_counter around the ctypes call, host arrays in, host arrays out, synchronous); the
median of --calls calls is reported, kernel times come from the handle's HIP-event profile in a separate set of calls.
Databases: kfdb_cases.make_database(n, 1800 words, 10^6-word vocabulary), i.e. KITTI-00-like BowVectors; queries are frames
seen from places of the trajectory.  One JSON line on stdout; --out merges the result into a JSON file under its mode's key.
Under rocprofv3 run it with a small --calls and --no-profile (events and the profiler's own tracing do not mix well).
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
from orb_slam3_rgbl_amd import kfdb_cases  # noqa: E402


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


def queries_for(db, n):
    step = max(1, db["n_places"] // n)
    return [kfdb_cases.make_query(db, (k * step) % db["n_places"], seed=k) for k in range(n)]


def bench_gpu(args):
    try:
        import torch  # noqa: F401  (whichever HIP runtime is mapped first serves the process; see tests/conftest.py)
    except ImportError:
        pass
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    lib = L.load()
    out = {}
    for n in args.sizes:
        db = kfdb_cases.make_database(n, args.words, args.vocab, seed=77, n_maps=2)
        dev = F.KeyFrameDatabase(db["n_vocab"], lib=lib)
        t0 = time.perf_counter()
        for e in db["entries"]:
            dev.add(e["kf_id"], e["map_id"], e["word_id"], e["word_val"])
        add_us = (time.perf_counter() - t0) / n * 1e6
        n_alive, n_words = dev.size()
        row = dict(entries=n_alive, words=n_words, add_us_per_key_frame=round(add_us, 1),
                   id_bytes=4 * n_words, value_bytes=8 * n_words)
        for Q in (1, 16):
            qs = queries_for(db, Q)
            off = np.zeros(Q + 1, np.int32)
            off[1:] = np.cumsum([len(q[0]) for q in qs])
            wid = np.ascontiguousarray(np.concatenate([q[0] for q in qs]), np.uint32)
            wval = np.ascontiguousarray(np.concatenate([q[1] for q in qs]), np.float64)
            kf, words = np.zeros((Q, n), np.int64), np.zeros((Q, n), np.int32)
            score, scored = np.zeros((Q, n), np.float32), np.zeros((Q, n), np.uint8)
            ns, mx, mn = np.zeros(Q, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32)
            if Q == 1:
                qin = L.KfdbQueryInput(len(wid), L.ptr(wid).value, L.ptr(wval).value, 0, None, 0)
                qout = L.KfdbQueryOutput(n, L.ptr(kf).value, L.ptr(words).value, L.ptr(score).value, L.ptr(scored).value, 0, 0, 0)
                a = (dev.h, C.byref(qin), C.byref(qout))
                fn = lambda: lib.rgbl_kfdb_query(*a)  # noqa: E731
            else:
                a = (dev.h, Q, L.ptr(off), L.ptr(wid), L.ptr(wval), None, None, None, n, L.ptr(kf), L.ptr(words), L.ptr(score),
                     L.ptr(scored), L.ptr(ns), L.ptr(mx), L.ptr(mn))
                fn = lambda: lib.rgbl_kfdb_query_batch(*a)  # noqa: E731
            assert fn() == 0, lib.rgbl_last_error()
            call = median_us(fn, args.calls)
            r = dict(call=call, per_query_us=round(call["median_us"] / Q, 1), query_words=int(off[Q]) // Q,
                     sharing=int(qout.n_share if Q == 1 else ns.mean()), scored=int(scored.sum()) // Q)
            if not args.no_profile:
                dev.profile(True)
                for _ in range(50):
                    fn()
                prof = dev.profile_read()
                dev.profile(False)
                r["kernels_us"] = {k: round(ms / max(cnt, 1) * 1e3, 1) for k, (ms, cnt) in prof.items()}
                r["kernels_total_us"] = round(sum(r["kernels_us"].values()), 1)
            row["Q%d" % Q] = r
        out["n%d" % n] = row
        dev.close()
    return dict(what="rgbl_kfdb_query (Q1) / rgbl_kfdb_query_batch (Q16): host arrays in, lKFsSharingWords + scores out, synchronous; "
                     "median of %d calls; kernels_us from HIP events on the handle's stream" % args.calls, **out)


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
    import kfdb_golden as kg
    lib = kg.build_reference_glue()
    out = {}
    fid = 1
    for n in args.sizes:
        db = kfdb_cases.make_database(n, args.words, args.vocab, seed=77, n_maps=2)
        be = kg.ReferenceBackend(db["n_vocab"], lib)
        for e in db["entries"]:
            be.add(e["kf_id"], e["map_id"], e["word_id"], e["word_val"])
        wid, wval = queries_for(db, 1)[0]
        wid, wval = np.ascontiguousarray(wid, np.uint32), np.ascontiguousarray(wval, np.float64)
        cand = np.zeros(n + 1, np.int64)
        t = []
        for k in range(args.calls + 3):
            fid += 1
            nc = lib.ref_kfdb_reloc(be.h, fid, len(wid), wid.ctypes.data_as(C.c_void_p), wval.ctypes.data_as(C.c_void_p), 0,
                                    cand.ctypes.data_as(C.c_void_p), len(cand))
            if k >= 3:
                t.append(lib.ref_kfdb_last_call_seconds(be.h) * 1e6)
        t = np.array(t)
        out["n%d" % n] = dict(entries=n, candidates=int(nc), median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), calls=len(t))
        be.close()
    return dict(what="the reference's own KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc and DBoW2 compiled "
                     "unmodified, -O2, one thread), timed inside the glue around the call itself; same databases and first query as the "
                     "device rows; no covisibility lists, so the tail after the scoring is a few list operations",
                host_cpu=cpu_model(), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,1500,5000")
    ap.add_argument("--words", type=int, default=1800)
    ap.add_argument("--vocab", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",")]
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
