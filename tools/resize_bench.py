"""What the image resize (cv::resize to Camera.newWidth / newHeight, System.cc:269-271, 349-351, 486-489, 557-560) costs on the
device, two ways, at the reference's EuRoC sizes 752 x 480 -> 600 x 350:

(a) kernel time per batch of rgbl_resize_batch_device (k_resize_image): HIP events on the extractor's stream, C = 1 and 3,
    B = 1 and 64.  Algorithmic bytes from shapes: B x C x (sw sh + dw dh); their rate as a share of a device-to-device copy
    ceiling measured in the same run (bytes read + written per second).  At B = 1 a launch moves 0.57 MB: that row is the
    latency of one launch in a back-to-back stream, not a bandwidth figure.
(b) the host-pointer leg at C = 1: rgbl_resize (upload, kernel, download, synchronous) beside the scalar CPU restatement (the
    oracle's cv::resize, one host core) on the same image; median of --calls calls, both legs twice, interleaved.  The CPU row is
    the SCALAR restatement: a SIMD OpenCV would be several times faster.

    python tools/resize_bench.py [--calls 300] [--out profiles/resize_calls.json]     on the MI355X

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

SIZES = (752, 480, 600, 350)


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


def kernel_leg(torch, dev, lib, F, ex, stream, ceiling, channels, batch, reps=7):
    import resize_ref as R
    sw, sh, dw, dh = SIZES
    inner = 50 if batch >= 8 else 200
    rs = F.Resizer((sw, sh), (dw, dh), lib=lib)
    info = rs.info()
    sstride, dstride = (sw * channels + 3) & ~3, (dw * channels + 3) & ~3
    sframe, dframe = sstride * sh, dstride * dh
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    src = torch.randint(0, 256, (batch * sframe,), dtype=torch.uint8, device=dev, generator=g)
    dst = torch.zeros(batch * dframe, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def run():
        rs.resize_batch_device(ex, src.data_ptr(), batch, channels, sstride, sframe, dst.data_ptr(), dstride, dframe)
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
    # the last frame against the restatement, so that the timed kernel is known to compute the right thing at this size
    f = batch - 1
    host = src[f * sframe:(f + 1) * sframe].cpu().numpy().reshape(sh, sstride)[:, :sw * channels]
    img = host if channels == 1 else host.reshape(sh, sw, channels)
    got = dst[f * dframe:(f + 1) * dframe].cpu().numpy().reshape(dh, dstride)[:, :dw * channels]
    same = bool(np.array_equal(got.reshape(dh, dw) if channels == 1 else got.reshape(dh, dw, channels), R.resize(img, dw, dh)))
    ms = float(np.median(times))
    alg = batch * channels * (sw * sh + dw * dh)
    rate = alg / (ms * 1e-3) / 1e9
    rs.close()
    del src, dst
    return dict(src="%dx%d" % (sw, sh), dst="%dx%d" % (dw, dh), channels=channels, batch=batch, table_bytes=info["table_bytes"],
                launches_per_window=inner, ms_per_batch=round(ms, 5), ms_min=round(min(times), 5), ms_max=round(max(times), 5),
                us_per_frame=round(ms * 1e3 / batch, 3), algorithmic_bytes=alg, achieved_GBps=round(rate, 1),
                share_of_copy_ceiling=round(rate / ceiling, 3), last_frame_equals_restatement=same)


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


def host_leg(lib, F, O, RC, calls):
    sw, sh, dw, dh = SIZES
    raw = RC.raw_image(sw, sh, 1)
    rs = F.Resizer((sw, sh), (dw, dh), lib=lib)
    same = bool(np.array_equal(rs.resize(raw), O.resize_linear(raw, dw, dh)))
    legs = {"rgbl_resize": lambda: rs.resize(raw), "cpu_restatement": lambda: O.resize_linear(raw, dw, dh)}
    r = dict(src="%dx%d" % (sw, sh), dst="%dx%d" % (dw, dh), channels=1, results="rgbl_resize == the oracle's cv::resize" if same else "MISMATCH")
    for run in (1, 2):
        for name, fn in legs.items():
            r["%s_run%d" % (name, run)] = stats_us(fn, calls if "cpu" not in name else max(calls // 6, 20))
    med = lambda k: [r["%s_run%d" % (k, i)]["median_us"] for i in (1, 2)]  # noqa: E731
    r["rgbl_resize_us"] = round(min(med("rgbl_resize")), 1)
    r["cpu_restatement_us"] = round(min(med("cpu_restatement")), 1)
    r["note"] = ("rgbl_resize is upload + kernel + download + synchronise on pageable host memory; the CPU row is the scalar restatement on "
                 "one core: a SIMD OpenCV would be several times faster")
    rs.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--kernels-only", action="store_true", help="part (a) alone: what a counter pass runs")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch  # first: whichever HIP runtime is mapped first serves the process (tests/conftest.py)
    from oracle import oracle_py as O
    from orb_slam3_rgbl_amd import _lib as L, frontend as F
    import resize_cases as RC
    lib = L.load()
    if lib.rgbl_device_count() < 1:
        raise SystemExit("resize_bench: no HIP device visible; nothing is measured without one")
    dev = torch.device("cuda", 0)
    doc = dict(what="cv::resize on the device (csrc/resize.hip): (a) kernel ms per batch from HIP events (median of 7 windows of back-to-back "
                    "launches), algorithmic bytes = B x C x (sw sh + dw dh), share of a 1 GiB device-to-device copy ceiling measured in this "
                    "run; (b) host-pointer legs, median of %d synchronous calls, both legs twice.  Parity: vs the restatement (= the oracle's "
                    "cv::resize at one channel), unpinned" % args.calls,
               date=time.strftime("%Y-%m-%d"))
    ceiling = copy_ceiling(torch, dev)
    doc["copy_ceiling_GBps"] = round(ceiling, 1)
    ex = RC.small_extractor(lib, max_batch=max(args.batches))   # the resize runs on an extractor's stream; its image size plays no part
    stream = torch.cuda.Stream(device=dev)
    L.check(lib, lib.rgbl_extractor_set_stream(ex.h, C.c_void_p(stream.cuda_stream)))
    doc["kernels"] = [kernel_leg(torch, dev, lib, F, ex, stream, ceiling, ch, b) for ch in (1, 3) for b in args.batches]
    stream.synchronize()
    L.check(lib, lib.rgbl_extractor_set_stream(ex.h, None))
    ex.close()
    if not args.kernels_only:
        O.build()
        doc["host_leg"] = host_leg(lib, F, O, RC, args.calls)
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
