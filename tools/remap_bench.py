"""What the stereo rectification (cv::remap, System.cc:260-268) costs on the device, two ways:

(a) kernel time per batch of rgbl_remap_batch_device (k_remap_linear, and k_remap_gather on a random map): HIP events on the
    extractor's stream, B = 64 and 512, 752 x 480 C = 1 and 1241 x 376 C = 3, the smooth map of tests/remap_cases.py (rotation
    + radial distortion).  Algorithmic bytes from shapes: map storage once + B x (source + destination); their rate as a share
    of a device-to-device copy ceiling measured in the same run (bytes read + written per second).
(b) the host-pointer leg at 752 x 480 C = 1: rgbl_extract_rectified on the raw image against the parent's path to the same
    result - the scalar C++ restatement of cv::remap (tests/remap_ref.cpp) on one host core + rgbl_extract - and rgbl_extract
    alone on the pre-rectified image; median of --calls synchronous calls, every leg twice, interleaved.  The CPU row is the
    SCALAR restatement: a SIMD OpenCV would be several times faster.

    python tools/remap_bench.py [--calls 300] [--out profiles/remap_calls.json]     on the MI355X

One JSON line on stdout; --out writes the same document."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def copy_ceiling(torch, dev, gib=1, reps=6):
    n = gib << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev)
    dst = torch.empty(n, dtype=torch.uint8, device=dev)
    src.fill_(1)
    dst.copy_(src)
    torch.cuda.synchronize(dev)
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    del src, dst
    return 2.0 * n / (best * 1e-3) / 1e9


def kernel_leg(torch, dev, lib, L, F, RC, ex, stream, ceiling, w, h, channels, batch, kind, reps=7, inner=10):
    sw, sh = w, h
    if kind == "smooth":
        mx, my = RC.smooth_map(w, h, sw, sh, focal=45.0 * w / RC.DST_W)
    else:
        mx, my = RC.random_map(w, h, sw, sh)
    rect = F.Rectifier(mx, my, (sw, sh), lib=lib)
    info = rect.info()
    stride = (w * channels + 3) & ~3
    fstride = stride * h
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    src = torch.randint(0, 256, (batch * fstride,), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.zeros(batch * fstride, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def run():
        rect.remap_batch_device(ex, src.data_ptr(), batch, channels, stride, fstride, dst.data_ptr(), stride, fstride)
    times = []
    with torch.cuda.stream(stream):
        for _ in range(3):
            run()
        stream.synchronize()
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(inner):
                run()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b) / inner)
    # frame 0 against the restatement, so that the timed kernels are known to compute the right thing at this size
    import remap_ref as R
    host = src[:fstride].cpu().numpy().reshape(h, stride)[:, :w * channels]
    img = host if channels == 1 else host.reshape(h, w, channels)
    same = bool(np.array_equal(dst[:fstride].cpu().numpy().reshape(h, stride)[:, :w * channels].reshape(img.shape), R.remap(img, mx, my)))
    ms = float(np.median(times))
    alg = info["map_bytes"] + batch * 2 * w * h * channels
    rate = alg / (ms * 1e-3) / 1e9
    rect.close()
    del src, dst
    return dict(map=kind, width=w, height=h, channels=channels, batch=batch, staged_tiles=info["staged_tiles"], direct_tiles=info["direct_tiles"],
                map_bytes=info["map_bytes"], ms_per_batch=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                us_per_frame=round(ms * 1e3 / batch, 3), algorithmic_bytes=alg, achieved_GBps=round(rate, 1),
                share_of_copy_ceiling=round(rate / ceiling, 3), frame0_equals_restatement=same)


def stats_us(fn, calls, warmup=10):
    warmup = min(warmup, calls)
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e6)
    t = np.array(t)
    return dict(median_us=round(float(np.median(t)), 1), min_us=round(float(t.min()), 1), p90_us=round(float(np.percentile(t, 90)), 1))


def host_leg(lib, L, F, RC, calls, w=752, h=480):
    import remap_ref as R
    sw, sh = w, h
    raw = RC.raw_image(sw, sh, 1)
    mx, my = RC.smooth_map(w, h, sw, sh, focal=45.0 * w / RC.DST_W)
    rect = F.Rectifier(mx, my, (sw, sh), lib=lib)
    ex_new, ex_old, ex_pre = (F.ORBextractor(1000, 1.2, 8, 20, 7, w, h, lib=lib) for _ in range(3))
    pre = R.remap(raw, mx, my)
    k0, d0, _, g0 = ex_new.extract_rectified(rect, raw)
    k1, d1, _ = ex_old(RC.remap_cpp(raw, mx, my))
    same = bool(np.array_equal(g0, pre) and RC.same_keypoints(k0, k1) and np.array_equal(d0, d1))
    legs = {
        "extract_rectified": lambda: ex_new.extract_rectified(rect, raw),
        "cpu_restatement_plus_extract": lambda: ex_old(RC.remap_cpp(raw, mx, my)),
        "extract_prerectified": lambda: ex_pre(pre),
        "cpu_restatement_alone": lambda: RC.remap_cpp(raw, mx, my),
    }
    r = dict(width=w, height=h, channels=1, keypoints=len(k0), results="extract_rectified == restatement + rgbl_extract" if same else "MISMATCH")
    for run in (1, 2):
        for name, fn in legs.items():
            r["%s_run%d" % (name, run)] = stats_us(fn, calls if "cpu" not in name else max(calls // 6, 20))
    med = lambda k: [r["%s_run%d" % (k, i)]["median_us"] for i in (1, 2)]  # noqa: E731
    pre_m, new_m, cpu_m = med("extract_prerectified"), med("extract_rectified"), med("cpu_restatement_alone")
    r["extract_spread_us"] = round(abs(pre_m[0] - pre_m[1]), 1)
    r["device_rectification_cost_us"] = round(min(new_m) - max(pre_m), 1)
    r["cpu_restatement_us"] = round(min(cpu_m), 1)
    r["cost_outside_the_spread"] = bool(r["device_rectification_cost_us"] > r["extract_spread_us"])
    r["cost_below_the_cpu_row"] = bool(max(new_m) - min(pre_m) < min(cpu_m))
    r["note"] = "the CPU row is the scalar restatement on one core; a SIMD OpenCV would be several times faster"
    for o in (rect, ex_new, ex_old, ex_pre):
        o.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--kernels-only", action="store_true", help="part (a) alone: what a counter pass runs")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch  # first: whichever HIP runtime is mapped first serves the process (tests/conftest.py)
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    import remap_cases as RC
    lib = L.load()
    if lib.rgbl_device_count() < 1:
        raise SystemExit("remap_bench: no HIP device visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    doc = dict(what="cv::remap on the device (csrc/rectify.hip): (a) kernel ms per batch from HIP events (median of 7 windows of 10 launches), "
                    "algorithmic bytes = map storage + B x (source + destination), share of a 1 GiB device-to-device copy ceiling measured in "
                    "this run; (b) host-pointer legs, median of %d synchronous calls, every leg twice" % args.calls,
               date=time.strftime("%Y-%m-%d"))
    ceiling = copy_ceiling(torch, dev)
    doc["copy_ceiling_GBps"] = round(ceiling, 1)
    ex = RC.small_extractor(lib)   # rgbl_remap_batch_device runs on an extractor's stream; its image size plays no part
    stream = torch.cuda.Stream(device=dev)
    L.check(lib, lib.rgbl_extractor_set_stream(ex.h, C.c_void_p(stream.cuda_stream)))
    doc["kernels"] = []
    for (w, h, ch) in ((752, 480, 1), (1241, 376, 3)):
        for b in args.batches:
            doc["kernels"].append(kernel_leg(torch, dev, lib, L, F, RC, ex, stream, ceiling, w, h, ch, b, "smooth"))
    doc["kernels"].append(kernel_leg(torch, dev, lib, L, F, RC, ex, stream, ceiling, 752, 480, 1, args.batches[0], "random"))
    stream.synchronize()
    L.check(lib, lib.rgbl_extractor_set_stream(ex.h, None))
    ex.close()
    if not args.kernels_only:
        doc["host_leg"] = host_leg(lib, L, F, RC, args.calls)
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
