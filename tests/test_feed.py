"""Host-fed batches on the emulator: the variable-length projection (rgbl_depth_project_xyzi_varlen_batch_device) and the
feeder's protocol and results (rgbl_feeder_*, orb_slam3_rgbl_amd/feed.py).  The emulator runs streams in order: these are
logic checks, the overlap is judged on the MI355X (tools/feed_bench.py)."""
import ctypes as C

import numpy as np
import pytest

import feed_cases as fc
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import feed as FD
from orb_slam3_rgbl_amd import frontend as F

W, H = 160, 96
METHODS = [F.UPS_INVERSE_DILATION, F.UPS_AVERAGE_FILTERING, F.UPS_NEAREST_NEIGHBOR_PIXEL]


@pytest.mark.parametrize("method", METHODS)
def test_varlen_scan_lengths(emu_lib, method):
    for lengths in ([0], [1], [255], [256], [1023], [1025], [1025, 0, 255, 1, 1023, 256]):
        fc.varlen_batch(emu_lib, False, W, H, method, lengths)


@pytest.mark.parametrize("sparse", [False, True])
def test_varlen_sparse_and_dense(emu_lib, sparse):
    _, _, _, _, hits = fc.varlen_batch(emu_lib, False, W, H, F.UPS_INVERSE_DILATION, [700, 0, 1500, 256], sparse=sparse, seed=3)
    assert hits > 20


def test_varlen_against_the_oracle(emu_lib, oracle):
    O = oracle
    scans, kps, depth, ur, _ = fc.varlen_batch(emu_lib, False, W, H, F.UPS_INVERSE_DILATION, [900, 1400], seed=11)
    proj = fc.projection(emu_lib, W, H)
    P = O.make_depth_params(proj, method=F.UPS_INVERSE_DILATION, kernel=O.structuring_element(F.KERNEL_DIAMOND, 5, 5))
    for b in range(2):
        cloud = np.ascontiguousarray(np.concatenate([scans[b][:, :3].T, np.ones((1, len(scans[b])), np.float32)]))
        xy = np.stack([kps[b]["x"], kps[b]["y"]], 1).astype(np.float32)
        d, u, _, _ = O.depth(P, cloud, W, H, xy, kps[b]["x"].astype(np.float32))
        assert np.array_equal(fc.bits(depth[b]), fc.bits(d)) and np.array_equal(fc.bits(ur[b]), fc.bits(u))


def test_varlen_equals_fixed_n_batch(emu_lib):
    lib, B, n, k = emu_lib, 3, 800, 60
    scans = [fc.bin_scan(40 + b, n) for b in range(B)]
    packed = np.ascontiguousarray(np.concatenate(scans))
    offsets = np.arange(B + 1, dtype=np.int64) * n
    kp = np.stack([fc.keypoints(b, W, H, k) for b in range(B)])
    counts = np.full(B, k, np.int32)
    out = []
    for varlen in (False, True):
        dm = fc.make_depth(lib, W, H, F.UPS_INVERSE_DILATION, n, B, k)
        proc = np.zeros((B, H, W), np.float32)
        d, u = np.zeros((B, k), np.float32), np.zeros((B, k), np.float32)
        if varlen:
            L.check(lib, lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), L.ptr(offsets), B, n, W, H, L.ptr(proc)))
        else:
            L.check(lib, lib.rgbl_depth_project_xyzi_batch_device(dm.h, L.ptr(packed), B, n, 4 * n, W, H, L.ptr(proc)))
        L.check(lib, lib.rgbl_depth_gather_batch_device(dm.h, B, W, H, L.ptr(kp), L.ptr(counts), k, None, L.ptr(d), L.ptr(u)))
        L.check(lib, lib.rgbl_depth_sync(dm.h))
        out.append((proc, d, u))
        dm.close()
    for a, b in zip(*out):
        assert np.array_equal(fc.bits(a), fc.bits(b))
    assert (out[0][0] > 0).sum() > 50


def test_varlen_overflow_is_reported(emu_lib):
    lib = emu_lib
    dm = fc.make_depth(lib, W, H, F.UPS_INVERSE_DILATION, 600, 2, 8)
    packed = np.ascontiguousarray(fc.bin_scan(1, 900))
    offsets = np.array([0, 300, 900], np.int64)  # the second scan holds 600 points, the call says 400
    L.check(lib, lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), L.ptr(offsets), 2, 400, W, H, None))
    assert lib.rgbl_depth_sync(dm.h) == L.ERR_OVERFLOW
    assert b"max_n" in lib.rgbl_last_error()
    assert lib.rgbl_depth_sync(dm.h) == L.RGBL_OK  # reported once, then cleared
    L.check(lib, lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), L.ptr(offsets), 2, 600, W, H, None))
    assert lib.rgbl_depth_sync(dm.h) == L.RGBL_OK
    # arguments the handle cannot take
    assert lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), L.ptr(offsets), 2, 601, W, H, None) == L.ERR_INVALID
    assert lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), L.ptr(offsets), 3, 100, W, H, None) == L.ERR_INVALID
    assert lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, L.ptr(packed), None, 2, 100, W, H, None) == L.ERR_INVALID
    dm.close()


def make_feeder(lib, max_batch=3, max_points=2000, slots=2, channels=3, **kw):
    ex = F.ORBextractor(300, 1.2, 4, 20, 7, 320, 200, max_batch=max_batch, lib=lib)
    dm = F.DepthModule(fc.projection(lib, 320, 200), 320, 200, max_points=max_points, max_keypoints=ex.max_keypoints,
                       max_batch=max_batch, lib=lib)
    fd = FD.HostFeeder(ex, dm, channels=channels, max_batch=max_batch, max_points=max_points, slots=slots, lib=lib, **kw)
    return ex, dm, fd


def fill_batch(fd, slot, lengths, seed=0):
    imgs = fc.colour_frames(seed, 320, 200, len(lengths), fd.channels)
    for b, n in enumerate(lengths):
        fd.fill(slot, b, imgs[b], fc.bin_scan(seed + b, n))


def test_feeder_protocol(emu_lib):
    lib = emu_lib
    ex, dm, fd = make_feeder(lib, max_batch=3, max_points=2000, slots=2, max_points_batch=3000)
    assert fd.pinned_bytes > 3 * 320 * 200 * 3 * 2
    s0 = fd.acquire()
    s1 = C.c_int()
    assert lib.rgbl_feeder_acquire(fd.h, C.byref(s1)) == L.RGBL_OK  # ring order
    assert (s0, s1.value) == (0, 1)
    # slot 0 is still being filled: the ring comes back to it
    assert lib.rgbl_feeder_acquire(fd.h, C.byref(C.c_int())) == L.ERR_INVALID
    # scans are reserved in frame order, within the feeder's room
    p = C.c_void_p()
    assert lib.rgbl_feeder_scan(fd.h, 0, 1, 10, C.byref(p)) == L.ERR_INVALID
    assert lib.rgbl_feeder_scan(fd.h, 0, 0, 2001, C.byref(p)) == L.ERR_CAPACITY
    assert lib.rgbl_feeder_submit(fd.h, 0, 1) == L.ERR_INVALID  # unfilled: no scan reserved
    fd.scan_view(0, 0, 2000)
    assert lib.rgbl_feeder_scan(fd.h, 0, 1, 1001, C.byref(p)) == L.ERR_CAPACITY  # 3000 points per batch
    fd.scan_view(0, 1, 1000)
    assert lib.rgbl_feeder_scan(fd.h, 0, 2, 1, C.byref(p)) == L.ERR_CAPACITY
    fd.scan_view(0, 2, 0)
    assert lib.rgbl_feeder_image(fd.h, 0, 3, C.byref(p)) == L.ERR_INVALID
    assert lib.rgbl_feeder_submit(fd.h, 0, 4) == L.ERR_INVALID  # longer than max_batch
    assert lib.rgbl_feeder_submit(fd.h, 0, 2) == L.ERR_INVALID  # three scans reserved
    assert lib.rgbl_feeder_collect(fd.h, 0, None) == L.ERR_INVALID  # nothing submitted
    fd.submit(0, 3)
    assert lib.rgbl_feeder_submit(fd.h, 0, 3) == L.ERR_INVALID
    fill_batch(fd, 1, [500, 0])
    fd.submit(1, 2)
    assert lib.rgbl_feeder_acquire(fd.h, C.byref(C.c_int())) == L.ERR_INVALID  # slot 0: submitted, not collected
    r0 = fd.collect(0)
    assert len(r0) == 3
    assert lib.rgbl_feeder_collect(fd.h, 0, None) == L.ERR_INVALID  # collecting twice
    assert fd.acquire() == 0
    res, ev = fd.device_outputs(1)
    assert res.batch == 2 and ev.value
    assert len(fd.collect(1)) == 2
    fill_batch(fd, 0, [10])
    fd.submit(0, 1)
    fd.close()  # destroys with a batch in flight
    # feeders that do not fit their handles
    for field, value in (("max_batch", 4), ("max_points", 2001), ("slots", 1), ("channels", 2), ("n_dist", 3)):
        cfg = L.FeederCfg(3, 1, 3, 2000, 0, 2)
        setattr(cfg, field, value)
        if field == "n_dist":
            cfg.dist[0] = 0.1
        h = C.c_void_p()
        assert lib.rgbl_feeder_create(C.byref(cfg), ex.h, dm.h, C.byref(h)) == L.ERR_INVALID, field
    dm_other = F.DepthModule(fc.projection(lib, 320, 200), 320, 208, max_points=2000, max_batch=3, lib=lib)
    h = C.c_void_p()
    assert lib.rgbl_feeder_create(C.byref(L.FeederCfg(3, 1, 3, 2000, 0, 2)), ex.h, dm_other.h, C.byref(h)) == L.ERR_INVALID
    for o in (ex, dm, dm_other):
        o.close()


@pytest.mark.parametrize("channels,blue_first", [(3, 1), (1, 0), (4, 0)])
def test_feeder_equals_single_frame_calls(emu_lib, channels, blue_first):
    stats = fc.feeder_vs_single(emu_lib, 320, 200, 300, 4, channels, blue_first, [[1200, 0, 700], [1500, 256], [900, 1, 1023]],
                                max_points=1500, slots=2)
    assert sum(n for n, _ in stats) > 200 and sum(d for _, d in stats) > 5


def test_feeder_undistorts(emu_lib):
    K = (718.856 * 320 / 1241, 718.856 * 320 / 1241, 160.0, 100.0)
    stats = fc.feeder_vs_single(emu_lib, 320, 200, 300, 4, 3, 1, [[1000, 800], [1200]], max_points=1200, slots=2, K=K,
                                dist=(-0.28, 0.07, 0.0002, 0.00002, 0.0))
    assert sum(d for _, d in stats) > 5


def test_feeder_undistortion_needs_the_intrinsics(emu_lib):
    ex = F.ORBextractor(300, 1.2, 4, 20, 7, 320, 200, lib=emu_lib)
    dm = F.DepthModule(fc.projection(emu_lib, 320, 200), 320, 200, max_points=100, max_keypoints=ex.max_keypoints, lib=emu_lib)
    with pytest.raises(ValueError):
        FD.HostFeeder(ex, dm, max_points=100, slots=2, dist=(-0.28, 0.07, 0.0, 0.0), lib=emu_lib)
    ex.close()
    dm.close()
