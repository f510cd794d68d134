"""Fed throughput: KITTI-size BGR frames with 115 - 130 k-point scans (seeded) from host memory through rgbl_feeder
(orb_slam3_rgbl_amd/feed.py), next to what the link and the resident path allow, measured in the same run.

    python tools/feed_bench.py [--batch 64 128] [--slots 3] [--steps 12] [--warmup 3] [--threads 8]

One JSON line per batch size:
  fed_fps             steady-state frames/s, inputs already in the slots (a caller that decodes / freads into them)
  pageable_fps        the same with up to --threads host threads copying every frame from ordinary (pageable) arrays first
  h2d_bytes_per_frame image + scan + offset bytes the feeder uploads per frame; h2d_gbs = fed_fps * that
  ceiling_gbs         one page-locked hipMemcpyAsync of a whole batch's bytes (torch non_blocking copy), and ceiling_fps /
                      fed_vs_ceiling = what that link rate allows per frame and the fraction of it reached
  resident_fps        the same cvtColor + extraction + varlen projection + gather on device-resident copies of the frames;
                      fed_vs_resident = fed_fps / resident_fps
  pinned_bytes        page-locked bytes the feeder holds
  parity              frame 0 of one batch against rgbl_extract_color + rgbl_depth_compute_xyzi (bit-exact)
Run under `rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/feed_bench.py ...` (no counters) to see whether
batch k + 1's input copies overlap batch k's kernels.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import torch  # noqa: F401  (first: its HIP runtime serves the process, as in bench.py)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orb_slam3_rgbl_amd import _lib as L  # noqa: E402
from orb_slam3_rgbl_amd import feed as FD  # noqa: E402
from orb_slam3_rgbl_amd import frontend as F  # noqa: E402
from orb_slam3_rgbl_amd import synth  # noqa: E402

W, H, MAXP = synth.KITTI_W, synth.KITTI_H, 130000


def frames(B, seed=0):
    seq = synth.Sequence(seed, W, H, n_frames=min(B, 16))
    rng = np.random.default_rng(seed)
    imgs, scans = [], []
    base = synth.lidar_scan(seed).T.copy()
    for b in range(B):
        g = seq.frame(b % 16)
        imgs.append(np.ascontiguousarray(np.stack([g, np.roll(g, 2 + b, 1), 255 - g], -1)))
        n = int(rng.integers(115000, MAXP + 1))
        s = base[rng.integers(0, base.shape[0], n)].astype(np.float32)
        s[:, 3] = rng.random(n)
        scans.append(np.ascontiguousarray(s))
    return imgs, scans


def fed_rate(fd, imgs, scans, steps, warmup, threads=0):
    B = len(imgs)
    pool = ThreadPoolExecutor(threads) if threads else None
    lens = [len(s) for s in scans]
    # inputs land in every slot once; later batches reserve the same scans again (zero-copy decode: data already in place)
    pending = []
    for _ in range(fd.slots):
        s = fd.acquire()
        for b in range(B):
            fd.fill(s, b, imgs[b], scans[b])
        fd.submit(s, B)
        pending.append(s)
    t0, done = None, 0
    for k in range(warmup + steps):
        fd.collect(pending.pop(0))
        if k == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        s = fd.acquire()
        views = [(fd.scan_view(s, b, lens[b]), fd.image_view(s, b)) for b in range(B)]
        if pool:
            def copy(b):
                np.copyto(views[b][0], scans[b])
                np.copyto(views[b][1], imgs[b])
            list(pool.map(copy, range(B)))
        fd.submit(s, B)
        pending.append(s)
        if k >= warmup:
            done += B
    for s in pending:
        fd.collect(s)
    dt = time.perf_counter() - t0
    if pool:
        pool.shutdown()
    return done / dt


def ceiling(nbytes, reps=10):
    src = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        dst.copy_(src, non_blocking=True)
    b.record()
    b.synchronize()
    return nbytes * reps / (a.elapsed_time(b) * 1e-3) / 1e9


def resident_rate(lib, ex, dm, imgs, scans, steps, warmup):
    B, cap = len(imgs), ex.max_keypoints
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    d_img = torch.from_numpy(np.stack(imgs)).cuda()
    d_gray = torch.empty(B * W * H + 64, dtype=torch.uint8, device="cuda")
    d_scan = torch.from_numpy(np.concatenate(scans)).cuda()
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)).cuda()
    kp = torch.empty((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device="cuda")
    n, mono = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    depth, ur = torch.empty((B, cap), device="cuda"), torch.empty((B, cap), device="cuda")
    es, ds = C.c_void_p(lib.rgbl_extractor_stream(ex.h)), C.c_void_p(lib.rgbl_depth_stream(dm.h))
    ev = C.c_void_p()
    L.check(lib, lib.rgbl_event_create(C.byref(ev)))
    max_n = max(len(s) for s in scans)
    torch.cuda.synchronize()
    t0 = None
    for k in range(warmup + steps):
        if k == warmup:
            L.check(lib, lib.rgbl_extractor_sync(ex.h))
            L.check(lib, lib.rgbl_depth_sync(dm.h))
            t0 = time.perf_counter()
        L.check(lib, lib.rgbl_cvt_gray_batch_device(ex.h, p(d_img), B, 3, 1, W, H, 3 * W, 3 * W * H, p(d_gray), W, W * H))
        L.check(lib, lib.rgbl_extract_batch_device(ex.h, p(d_gray), B, W, H, W, W * H, 0, 0, p(kp), p(desc), cap, p(n), p(mono)))
        L.check(lib, lib.rgbl_event_record(ev, es))
        L.check(lib, lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, p(d_scan), p(d_off), B, max_n, W, H, None))
        L.check(lib, lib.rgbl_event_wait(ds, ev))
        L.check(lib, lib.rgbl_depth_gather_batch_device(dm.h, B, W, H, p(kp), p(n), cap, None, p(depth), p(ur)))
        L.check(lib, lib.rgbl_stream_wait(es, ds))  # the next batch's extraction overwrites the keypoints the gather reads
    L.check(lib, lib.rgbl_extractor_sync(ex.h))
    L.check(lib, lib.rgbl_depth_sync(dm.h))
    dt = time.perf_counter() - t0
    lib.rgbl_event_destroy(ev)
    return steps * B / dt


def parity(lib, fd, imgs, scans):
    s = fd.acquire()
    for b in range(len(imgs)):
        fd.fill(s, b, imgs[b], scans[b])
    fd.submit(s, len(imgs))
    got = fd.collect(s)[0]
    ex1 = F.ORBextractor(2000, 1.2, 8, 20, 7, W, H, lib=lib)
    dm1 = F.DepthModule(F.projection_matrix(synth.KITTI_K, synth.KITTI_TR, lib), W, H, max_points=MAXP,
                        max_keypoints=ex1.max_keypoints, lib=lib)
    cap = ex1.max_keypoints
    kp, desc = np.zeros(cap, L.KP_DTYPE), np.zeros((cap, 32), np.uint8)
    n, mono = C.c_int(), C.c_int()
    L.check(lib, lib.rgbl_extract_color(ex1.h, L.ptr(imgs[0]), 3, 1, W, H, 3 * W, 0, 0, L.ptr(kp), L.ptr(desc), cap, C.byref(n),
                                        C.byref(mono), None, 0))
    k = n.value
    xy = np.ascontiguousarray(np.stack([kp["x"][:k], kp["y"][:k]], 1))
    un = np.ascontiguousarray(kp["x"][:k])
    d, u = np.zeros(k, np.float32), np.zeros(k, np.float32)
    L.check(lib, lib.rgbl_depth_compute_xyzi(dm1.h, L.ptr(scans[0]), len(scans[0]), W, H, L.ptr(xy), L.ptr(un), k, L.ptr(d), L.ptr(u),
                                             None, None))
    ok = (got["n"] == k and np.array_equal(got["kp"].view(np.uint8), kp[:k].view(np.uint8)) and np.array_equal(got["desc"], desc[:k])
          and np.array_equal(got["depth"].view(np.uint32), d.view(np.uint32)) and np.array_equal(got["uright"].view(np.uint32), u.view(np.uint32)))
    ex1.close()
    dm1.close()
    return bool(ok), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    lib = L.load()
    for B in a.batch:
        imgs, scans = frames(B)
        ex = F.ORBextractor(2000, 1.2, 8, 20, 7, W, H, max_batch=B, lib=lib)
        dm = F.DepthModule(F.projection_matrix(synth.KITTI_K, synth.KITTI_TR, lib), W, H, max_points=MAXP,
                           max_keypoints=ex.max_keypoints, max_batch=B, lib=lib)
        fd = FD.HostFeeder(ex, dm, channels=3, blue_first=1, max_batch=B, max_points=MAXP, slots=a.slots, lib=lib)
        h2d = int(sum(i.nbytes for i in imgs) + sum(s.nbytes for s in scans) + 8 * (B + 1))
        ok, k0 = parity(lib, fd, imgs, scans)
        fed = fed_rate(fd, imgs, scans, a.steps, a.warmup)
        pageable = fed_rate(fd, imgs, scans, max(a.steps // 2, 3), 1, threads=a.threads)
        ceil_gbs = ceiling(h2d)
        pinned = fd.pinned_bytes
        fd.close()
        res = resident_rate(lib, ex, dm, imgs, scans, a.steps, a.warmup)
        per_frame = h2d / B
        print(json.dumps(dict(metric="fed_frames_per_s", batch=B, slots=a.slots, channels=3, fed_fps=round(fed, 1),
                              pageable_fps=round(pageable, 1), pageable_threads=a.threads, h2d_bytes_per_frame=int(per_frame),
                              h2d_gbs=round(fed * per_frame / 1e9, 2), ceiling_gbs=round(ceil_gbs, 2),
                              ceiling_fps=round(ceil_gbs * 1e9 / per_frame, 1), fed_vs_ceiling=round(fed * per_frame / (ceil_gbs * 1e9), 3),
                              resident_fps=round(res, 1), fed_vs_resident=round(fed / res, 3), pinned_bytes=int(pinned),
                              parity=ok, parity_keypoints=k0)), flush=True)
        ex.close()
        dm.close()


if __name__ == "__main__":
    main()
