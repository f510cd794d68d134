"""Shared cases of the host-fed batch tests (test_feed.py on the emulator, test_feed_gpu.py on the MI355X): variable-length
.bin scans, the varlen projection against one rgbl_depth_compute_xyzi call per scan, the feeder against the single-frame
host calls."""
import ctypes as C

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import feed as FD
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def projection(lib, w, h):
    K = synth.KITTI_K.copy()
    if w != synth.KITTI_W:
        K[0, 2], K[1, 2] = w / 2.0, h / 2.0
        K[0, 0] = K[1, 1] = 718.856 * w / synth.KITTI_W
    return F.projection_matrix(K, synth.KITTI_TR, lib)


def bin_scan(seed, n, n_az=1900):
    """n velodyne .bin records (x, y, z, reflectance), mostly in front of the camera, with repeated points (last one wins)."""
    cloud = synth.lidar_scan(seed, n_az=n_az).T.copy()
    rng = np.random.default_rng(seed + 5)
    front = cloud[(cloud[:, 0] > 2.0) & (np.abs(cloud[:, 1]) < cloud[:, 0])]
    pick = np.concatenate([front, cloud])
    pts = pick[rng.integers(0, len(pick), n)] if n else np.zeros((0, 4), np.float32)
    if n > 4:
        pts[n // 2] = pts[n // 4]  # the same pixel twice: the later record wins
        pts[n // 2, 0] += 0.5
    pts = pts.astype(np.float32)
    pts[:, 3] = rng.random(n).astype(np.float32)  # reflectance: dropped by the loader
    return np.ascontiguousarray(pts)


def keypoints(seed, w, h, k):
    rng = np.random.default_rng(seed + 99)
    kp = np.zeros(k, L.KP_DTYPE)
    kp["x"] = rng.uniform(0, w - 1, k).astype(np.float32)
    kp["y"] = rng.uniform(0, h - 1, k).astype(np.float32)
    kp["x"][: k // 2] = np.floor(kp["x"][: k // 2])
    return kp


def make_depth(lib, w, h, method, max_points, max_batch, max_keypoints, sparse=False):
    dm = F.DepthModule(projection(lib, w, h), w, h, method=method, max_points=max_points, max_keypoints=max_keypoints,
                       max_batch=max_batch, lib=lib)
    if sparse:
        dm.set_sparse(True) if hasattr(dm, "set_sparse") else L.check(lib, lib.rgbl_depth_set_sparse(dm.h, 1))
    return dm


def single_depth(lib, w, h, method, scan, kp, sparse=False):
    """One rgbl_depth_compute_xyzi call: (mvDepth, mvuRight, ProcessedDepthMap or None)."""
    dm = make_depth(lib, w, h, method, max(len(scan), 1), 1, max(len(kp), 1), sparse)
    k = len(kp)
    xy = np.ascontiguousarray(np.stack([kp["x"], kp["y"]], 1).astype(np.float32))
    un = np.ascontiguousarray(kp["x"].astype(np.float32))
    d, ur = np.zeros(k, np.float32), np.zeros(k, np.float32)
    proc = None if (method == F.UPS_NEAREST_NEIGHBOR_PIXEL or sparse) else np.zeros((h, w), np.float32)
    L.check(lib, lib.rgbl_depth_compute_xyzi(dm.h, L.ptr(scan), len(scan), w, h, L.ptr(xy), L.ptr(un), k, L.ptr(d), L.ptr(ur), None,
                                             L.ptr(proc)))
    dm.close()
    return d, ur, proc


class DeviceArrays:
    """Device buffers for the varlen calls: numpy arrays on the emulator (its device memory is host memory), torch tensors
    on the GPU."""

    def __init__(self, gpu):
        self.gpu = gpu
        self.keep = []
        if gpu:
            import torch
            self.torch = torch

    def put(self, a):
        a = np.ascontiguousarray(a)
        if not self.gpu:
            self.keep.append(a)
            return a
        t = self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append((t, a.dtype, a.shape))
        return t

    def ptr(self, a):
        return L.ptr(a) if not self.gpu else C.c_void_p(a.data_ptr())

    def get(self, a, dtype, shape):
        if not self.gpu:
            return a
        return a.cpu().numpy().view(dtype).reshape(shape)

    def zeros(self, dtype, shape):
        return self.put(np.zeros(shape, dtype))


def varlen_batch(lib, gpu, w, h, method, lengths, sparse=False, seed=0, n_kp=120, max_n=None):
    """The varlen projection of len(lengths) scans + the batch gather against one single-frame call per scan."""
    B = len(lengths)
    scans = [bin_scan(seed + 7 * b, n) for b, n in enumerate(lengths)]
    kps = [keypoints(seed + b, w, h, n_kp) for b in range(B)]
    max_n = max(lengths) if max_n is None else max_n
    dm = make_depth(lib, w, h, method, max(max_n, 1), B, n_kp, sparse)
    D = DeviceArrays(gpu)
    packed = np.concatenate(scans + [np.zeros((1, 4), np.float32)])  # (+1 record: never an empty allocation)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    d_xyzi, d_off = D.put(packed), D.put(offsets)
    kp_all = np.zeros((B, n_kp), L.KP_DTYPE)
    for b in range(B):
        kp_all[b] = kps[b]
    d_kp, d_n = D.put(kp_all), D.put(np.full(B, n_kp, np.int32))
    dense = method != F.UPS_NEAREST_NEIGHBOR_PIXEL and not sparse
    d_proc = D.zeros(np.float32, (B, h, w)) if dense else None
    d_depth, d_ur = D.zeros(np.float32, (B, n_kp)), D.zeros(np.float32, (B, n_kp))
    L.check(lib, lib.rgbl_depth_project_xyzi_varlen_batch_device(dm.h, D.ptr(d_xyzi), D.ptr(d_off), B, max_n, w, h,
                                                                  D.ptr(d_proc) if dense else None))
    L.check(lib, lib.rgbl_depth_gather_batch_device(dm.h, B, w, h, D.ptr(d_kp), D.ptr(d_n), n_kp, None, D.ptr(d_depth), D.ptr(d_ur)))
    L.check(lib, lib.rgbl_depth_sync(dm.h))
    depth, ur = D.get(d_depth, np.float32, (B, n_kp)), D.get(d_ur, np.float32, (B, n_kp))
    proc = D.get(d_proc, np.float32, (B, h, w)) if dense else None
    hits = 0
    for b in range(B):
        d1, u1, p1 = single_depth(lib, w, h, method, scans[b], kps[b], sparse)
        assert np.array_equal(bits(depth[b]), bits(d1)), ("mvDepth", b, lengths[b])
        assert np.array_equal(bits(ur[b]), bits(u1)), ("mvuRight", b, lengths[b])
        if dense:
            assert np.array_equal(bits(np.nan_to_num(proc[b])), bits(np.nan_to_num(p1))), ("ProcessedDepthMap", b, lengths[b])
            if lengths[b] == 0:
                assert not (proc[b] > 0).any(), "an empty scan gives an empty depth map"
        hits += int((d1 > 0).sum())
    dm.close()
    return scans, kps, depth, ur, hits


def single_frame(lib, ex, dm, img, channels, blue_first, scan, K=None, dist=None):
    """rgbl_extract_color + (undistortion) + rgbl_depth_compute_xyzi of one frame: what the feeder must reproduce."""
    h, w = img.shape[:2]
    cap = ex.max_keypoints
    kp = np.zeros(cap, L.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n, mono = C.c_int(), C.c_int()
    stride = w * channels
    L.check(lib, lib.rgbl_extract_color(ex.h, L.ptr(np.ascontiguousarray(img)), channels, blue_first, w, h, stride, 0, 0, L.ptr(kp),
                                        L.ptr(desc), cap, C.byref(n), C.byref(mono), None, 0))
    k = n.value
    kp, desc = kp[:k].copy(), desc[:k].copy()
    xy = np.ascontiguousarray(np.stack([kp["x"], kp["y"]], 1).astype(np.float32))
    un_xy = None
    if dist is not None and len(dist) and dist[0] != 0:
        un_xy = np.zeros_like(xy)
        Ka, Da = np.asarray(K, np.float32), np.asarray(dist, np.float32)
        if k:
            L.check(lib, lib.rgbl_undistort_points(ex.h, L.ptr(xy), k, L.ptr(Ka), L.ptr(Da), len(Da), L.ptr(un_xy)))
    un_x = np.ascontiguousarray((un_xy if un_xy is not None else xy)[:, 0])
    d, ur = np.zeros(k, np.float32), np.zeros(k, np.float32)
    L.check(lib, lib.rgbl_depth_compute_xyzi(dm.h, L.ptr(scan), len(scan), w, h, L.ptr(xy), L.ptr(un_x), k, L.ptr(d), L.ptr(ur),
                                             None, None))
    return dict(n=k, mono=mono.value, kp=kp, desc=desc, depth=d, uright=ur, kpun_xy=un_xy)


def compare_frame(got, want, tag=""):
    assert got["n"] == want["n"], (tag, got["n"], want["n"])
    assert got["mono"] == want["mono"], tag
    assert np.array_equal(got["kp"].view(np.uint8), want["kp"].view(np.uint8)), (tag, "kp")
    assert np.array_equal(got["desc"], want["desc"]), (tag, "desc")
    assert np.array_equal(bits(got["depth"]), bits(want["depth"])), (tag, "depth")
    assert np.array_equal(bits(got["uright"]), bits(want["uright"])), (tag, "uright")
    if want["kpun_xy"] is not None:
        assert np.array_equal(bits(got["kpun_xy"]), bits(want["kpun_xy"])), (tag, "kpun_xy")
    else:
        assert "kpun_xy" not in got


def colour_frames(seed, w, h, count, channels):
    seq = synth.Sequence(seed, w, h, n_frames=count)
    out = []
    rng = np.random.default_rng(seed)
    for i in range(count):
        g = seq.frame(i)
        if channels == 1:
            out.append(np.ascontiguousarray(g))
            continue
        c = np.stack([g, np.roll(g, 3, 1), 255 - g] + ([rng.integers(0, 256, g.shape, dtype=np.uint8)] if channels == 4 else []), -1)
        out.append(np.ascontiguousarray(c.astype(np.uint8)))
    return out


def feeder_vs_single(lib, w, h, nfeatures, nlevels, channels, blue_first, batches, max_points, slots=3, method=F.UPS_INVERSE_DILATION,
                     K=None, dist=None, seed=0, sparse=False, depth_kwargs=None):
    """Runs `batches` (lists of scan lengths) through a HostFeeder and compares every frame with the single-frame calls.
    Returns the frames' keypoint and depth-hit counts."""
    max_batch = max(len(b) for b in batches)
    ex = F.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, w, h, max_batch=max_batch, lib=lib)
    cap = ex.max_keypoints
    kw = dict(method=method, max_points=max_points, max_keypoints=cap, max_batch=max_batch, lib=lib)
    kw.update(depth_kwargs or {})
    proj = projection(lib, w, h)
    dm = F.DepthModule(proj, w, h, **kw)
    if sparse:
        L.check(lib, lib.rgbl_depth_set_sparse(dm.h, 1))
    fd = FD.HostFeeder(ex, dm, channels=channels, blue_first=blue_first, max_batch=max_batch, max_points=max_points, slots=slots,
                       K=K, dist=dist, lib=lib)
    frames_in = []
    for k, lengths in enumerate(batches):
        imgs = colour_frames(seed + k, w, h, len(lengths), channels)
        frames_in.append([(imgs[b], bin_scan(seed + 31 * k + b, n)) for b, n in enumerate(lengths)])
    results = list(fd.run(frames_in))
    fd.close()
    # the same frames through the single-frame host calls on handles of their own
    ex1 = F.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, w, h, lib=lib)
    kw1 = dict(kw, max_batch=1, max_keypoints=ex1.max_keypoints)
    dm1 = F.DepthModule(proj, w, h, **kw1)
    stats = []
    for k, (fin, fout) in enumerate(zip(frames_in, results)):
        assert len(fin) == len(fout)
        for b, ((img, scan), got) in enumerate(zip(fin, fout)):
            want = single_frame(lib, ex1, dm1, img, channels, blue_first, scan, K, dist)
            compare_frame(got, want, (k, b))
            stats.append((got["n"], int((got["depth"] > 0).sum())))
    for o in (ex, dm, ex1, dm1):
        o.close()
    return stats
